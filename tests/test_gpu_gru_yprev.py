"""The previous-state layout of the GRU layer output (tt_gru_fwd_yprev / tt_gru_bwd_yprev,
option gru_yprev): row t of Y holds the state the step at t starts from, so dW_hh is a plain TN
GEMM. Nothing that is computed changes, so every comparison here is bit for bit (torch.equal)
against the default layout:

  forward   Yp[b, t] == Y[b, t-1] (dir 0) / Y[b, t+1] (dir 1), the row without a predecessor
            exact zeros (written by the call: every output is prefilled with NaN), hfinal == the
            default call's last state, S and X1 unchanged, sentinel rows untouched; T = 1 is
            the case where the only row of Y is the zero row;
  backward  gru_bwd_rows on (Y, tt_gru_bwd) and on (Yp, tt_gru_bwd_yprev): dgx, dgh, the carry
            buffer and the bias partials;
  dW_hh     the plain split-K GEMM on Yp against the time-shifted GEMM on Y;
  model     one training step with gru_yprev 1 and 0: outputs, loss and all 44 gradients, with
            dropout (both layers in the new layout), without (layer 0 falls back) and on shapes
            the layout does not cover (fp32, H 128), with the entry points that ran recorded.
"""
import contextlib
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import two_towers_amd as tta  # noqa: E402
from two_towers_amd import _lib, ops, towers  # noqa: E402
from two_towers_amd._lib import GruBwdRec, GruFwdRec, call, option, stream_ptr  # noqa: E402
from two_towers_amd.towers import gru_fwd_workspace  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
SENT = -777.0
NAN = float("nan")


@contextlib.contextmanager
def options(**kw):
    with contextlib.ExitStack() as st:
        for k, v in kw.items():
            st.enter_context(option(k, v))
        yield


def _shifted(Y, B, T, H):
    """[B*T, 2H] (fwd | rev) in the default layout -> the previous-state layout."""
    y = Y.reshape(B, T, 2 * H)
    yp = torch.zeros_like(y)
    yp[:, 1:, :H] = y[:, :-1, :H]
    yp[:, :-1, H:] = y[:, 1:, H:]
    return yp.reshape(B * T, 2 * H).contiguous()


def _zero_bits(t):
    return bool((t.contiguous().view(torch.int16) == 0).all())


# ------------------------------------------------------------------------------ forward

@functools.lru_cache(maxsize=None)
def _fwd_inputs(H, B, T, ntow):
    g = torch.Generator().manual_seed(7000 + H + 10 * T + ntow)
    out = []
    for _ in range(ntow):
        G = torch.randn(B * T, 6 * H, generator=g).to(BF16).to(DEV)
        whh = [(torch.randn(3 * H, H, generator=g) * H ** -0.5).to(BF16).to(DEV) for _ in range(2)]
        bhn = [(torch.randn(H, generator=g) * 0.5).to(DEV) for _ in range(2)]
        out.append((G, whh, bhn))
    return out


def _run_fwd(H, B, T, nrec, drop_p, yprev):
    ntow, BT = nrec // 2, B * T
    inp = _fwd_inputs(H, B, T, ntow)

    def buf(rows, cols):
        t = torch.full((rows + 1, cols), NAN, dtype=BF16, device=DEV)
        t[rows] = SENT
        return t
    Y = [buf(BT, 2 * H) for _ in range(ntow)]
    X1 = [buf(BT, 2 * H) for _ in range(ntow)] if drop_p > 0 else None
    S = [buf(BT, 4 * H) for _ in range(nrec)]
    F = [buf(B, 2 * H) for _ in range(ntow)]
    hs = torch.zeros(nrec, 2, B, H, dtype=torch.float32, device=DEV)
    recs = (GruFwdRec * nrec)()
    fin = (ctypes.c_void_p * nrec)()
    for i in range(nrec):
        ti, d = i // 2, i % 2
        G, whh, bhn = inp[ti]
        r = recs[i]
        r.g, r.whh, r.bhn = G[:, d * 3 * H:].data_ptr(), whh[d].data_ptr(), bhn[d].data_ptr()
        r.y, r.save = Y[ti][:, d * H:].data_ptr(), S[i].data_ptr()
        r.x1 = X1[ti][:, d * H:].data_ptr() if X1 is not None else None
        r.hstate, r.dir = hs[i].data_ptr(), d
        r.drop_seed, r.drop_col0, r.drop_row0 = 911 + 17 * ti, d * H, 5
        fin[i] = F[ti][:, d * H:].data_ptr()
    dtc = _lib.dtype_code(BF16)
    ws = gru_fwd_workspace(nrec, B, T, H, BF16, torch.device(DEV))
    assert ws is not None, "the column-split kernel does not apply to this shape"
    if yprev:
        assert _lib.load().tt_gru_yprev_supported(dtc, nrec, B, T, H, 6 * H, 2 * H) == 1
        call("tt_gru_fwd_yprev", dtc, recs, fin, nrec, B, T, H, 6 * H, 2 * H, 2 * H, drop_p, ws.data_ptr(), ws.numel(),
             stream_ptr())
    else:
        call("tt_gru_fwd", dtc, recs, nrec, B, T, H, 6 * H, 2 * H, drop_p, ws.data_ptr(), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0, "a column-split member wait timed out"
    return Y, X1, S, F


@pytest.mark.parametrize("drop_p", [0.1, 0.0])
@pytest.mark.parametrize("T", [3, 1])
@pytest.mark.parametrize("nrec", [2, 4])
@pytest.mark.parametrize("H,xs", [(256, 1), (512, 1), (512, 0)])
def test_column_split_forward_previous_state_layout(H, xs, nrec, T, drop_p):
    """gru_fwd_xcp at H 256, gru_fwd_xs and gru_fwd_xcp at H 512 (gru_fwd_xc = 2 forces them on
    B 70: groups with few or no rows), with and without the dropout copy."""
    B, BT = 70, 70 * T
    with options(gru_fwd_xc=2, gru_fwd_xs=xs):
        Y, X1, S, _ = _run_fwd(H, B, T, nrec, drop_p, False)
        Yp, X1p, Sp, F = _run_fwd(H, B, T, nrec, drop_p, True)
    for ti in range(nrec // 2):
        y = Y[ti][:BT].reshape(B, T, 2 * H)
        yp = Yp[ti][:BT].reshape(B, T, 2 * H)
        assert not torch.isnan(y.float()).any()
        # dir 0: row t holds h_{t-1}, zeros at t = 0; the last state is h_{T-1}
        assert torch.equal(yp[:, 1:, :H], y[:, :-1, :H])
        assert _zero_bits(yp[:, 0, :H]), "dir 0: the row of t = 0 is not exact zeros"
        assert torch.equal(F[ti][:B, :H], y[:, T - 1, :H])
        # dir 1: row t holds h_{t+1}, zeros at t = T-1; the last state is h_0
        assert torch.equal(yp[:, :-1, H:], y[:, 1:, H:])
        assert _zero_bits(yp[:, T - 1, H:]), "dir 1: the row of t = T-1 is not exact zeros"
        assert torch.equal(F[ti][:B, H:], y[:, 0, H:])
        if drop_p > 0:
            assert torch.equal(X1p[ti][:BT], X1[ti][:BT])
            assert bool((X1p[ti][BT] == SENT).all())
        assert bool((Yp[ti][BT] == SENT).all()), "Y: the row after B*T was written"
        assert bool((F[ti][B] == SENT).all()), "hfinal: the row after B was written"
    for i in range(nrec):
        assert torch.equal(Sp[i][:BT], S[i][:BT]), i
        assert bool((Sp[i][BT] == SENT).all())


def test_previous_state_layout_is_refused_where_unsupported():
    """Never another layout in place of the one asked for: fp32, H 136 and a call without the
    workspace are errors of the new entry points and 0 from the query."""
    lib = _lib.load()
    assert lib.tt_gru_yprev_supported(_lib.DT_F32, 4, 8192, 64, 512, 3072, 1024) == 0
    assert lib.tt_gru_yprev_supported(_lib.DT_BF16, 4, 8192, 64, 136, 6 * 136, 2 * 136) == 0
    assert lib.tt_gru_yprev_supported(_lib.DT_BF16, 4, 8192, 64, 512, 3072, 1024) == 1
    with options(gru_fwd_xc=0):
        assert lib.tt_gru_yprev_supported(_lib.DT_BF16, 4, 8192, 64, 512, 3072, 1024) == 0
    with options(gru_bwd_persist=0):
        assert lib.tt_gru_yprev_supported(_lib.DT_BF16, 4, 8192, 64, 512, 3072, 1024) == 0
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    recs = (GruFwdRec * 1)()
    r = recs[0]
    r.g = r.whh = r.bhn = r.y = r.save = r.hstate = x.data_ptr()
    assert lib.tt_gru_fwd_yprev(_lib.DT_BF16, recs, None, 1, 1, 1, 512, 3072, 1024, 1024, 0.0, None, 0, None) == _lib.TT_EINVAL
    brecs = (GruBwdRec * 1)()
    assert lib.tt_gru_bwd_yprev(_lib.DT_F32, brecs, 1, 1, 1, 512, 1024, 4096, 1024, None) == _lib.TT_EINVAL


# ----------------------------------------------------------------------------- backward

@pytest.mark.parametrize("mode", ["dy", "dfinal", "both"])
@pytest.mark.parametrize("T", [4, 1])
@pytest.mark.parametrize("H", [256, 512])
def test_row_owning_backward_reads_the_previous_state_layout(H, T, mode):
    """gru_bwd_rows<H>: B 130 is one 128-row tile and a 2-row tail."""
    B, nrec = 130, 2
    BT = B * T
    g = torch.Generator().manual_seed(8000 + H + T)
    S = [torch.randn(BT, 4 * H, generator=g).to(BF16).to(DEV) for _ in range(nrec)]
    Y = torch.tanh(torch.randn(BT, 2 * H, generator=g)).to(BF16).to(DEV)
    whh = [(torch.randn(3 * H, H, generator=g) * H ** -0.5).to(BF16).to(DEV) for _ in range(2)]
    dY = torch.randn(BT, 2 * H, generator=g).to(BF16).to(DEV)
    dF = torch.randn(B, 2 * H, generator=g).to(DEV)
    lib = _lib.load()
    dtc = _lib.dtype_code(BF16)
    assert lib.tt_gru_bwd_launches(dtc, 2, H) == 1
    nbr = lib.tt_gru_bias_rows(B)
    outs = []
    for yprev in (0, 1):
        Yin = _shifted(Y, B, T, H) if yprev else Y
        dG = torch.full((BT + 1, 8 * H), SENT, dtype=BF16, device=DEV)
        dhs = torch.zeros(nrec, 2, B, H, dtype=BF16, device=DEV)
        part = torch.full((nrec, nbr, 4 * H), 1e30, dtype=torch.float32, device=DEV)
        recs = (GruBwdRec * nrec)()
        for d in range(nrec):
            r = recs[d]
            r.save, r.y, r.whh = S[d].data_ptr(), Yin[:, d * H:].data_ptr(), whh[d].data_ptr()
            r.dy = dY[:, d * H:].data_ptr() if mode != "dfinal" else None
            r.dfinal = dF[:, d * H:].data_ptr() if mode != "dy" else None
            r.dgx, r.dgh = dG[:, d * 3 * H:].data_ptr(), dG[:, 6 * H + d * H:].data_ptr()
            r.dhstate, r.dbias_part, r.dir = dhs[d].data_ptr(), part[d].data_ptr(), d
        call("tt_gru_bwd_yprev" if yprev else "tt_gru_bwd", dtc, recs, nrec, B, T, H, 2 * H, 8 * H, 2 * H, stream_ptr())
        torch.cuda.synchronize()
        outs.append((dG, dhs, part))
    (g0, h0, p0), (g1, h1, p1) = outs
    assert not torch.isnan(g0.float()).any() and bool((g0[BT] == SENT).all()) and bool((g0[:BT] != SENT).any())
    assert torch.equal(g0[:, :6 * H], g1[:, :6 * H]), "dgx"
    assert torch.equal(g0[:, 6 * H:], g1[:, 6 * H:]), "dgh"
    assert torch.equal(h0, h1), "dhstate"
    assert torch.equal(p0, p1), "bias partials"


# -------------------------------------------------------------------------------- dW_hh

@pytest.mark.parametrize("T,Bsz", [(64, 32), (128, 16), (64, 256)])
def test_wgrad_hh_plain_gemm_on_previous_state_layout(T, Bsz):
    """dW_hh (split-column A, split-K on 256-row tiles): the plain TN GEMM on Yp against the
    time-shifted GEMM on Y (the buffer form of the shift: T is a whole number of K-tiles)."""
    H, K = 256, T * Bsz
    g = torch.Generator().manual_seed(9000 + T + Bsz)
    dG = torch.randn(K, 8 * H, generator=g).to(BF16).to(DEV)
    Y = torch.randn(K, 2 * H, generator=g).to(BF16).to(DEV)
    Yp = _shifted(Y, Bsz, T, H)
    a = [dG[:, d * 3 * H:] for d in range(2)]
    a_hi = [dG[:, 6 * H + d * H:] for d in range(2)]
    assert ops.gemm_splits(3 * H, H, K, 2, BF16) > 1

    def run(b, **kw):
        C = [torch.full((3 * H, H), NAN, device=DEV) for _ in range(2)]
        ops.gemm(a, b, C, m=3 * H, n=H, k=K, lda=8 * H, ldb=2 * H, ldc=H, a_kouter=True, b_kouter=True, dtype=BF16,
                 out_dtype=torch.float32, a_hi=a_hi, a_split=2 * H, **kw)
        return C

    with options(gemm_buf=1):
        shifted = run([Y[:, d * H:] for d in range(2)], bshift=[-1, 1], seq_t=T)
        plain = run([Yp[:, d * H:] for d in range(2)])
    torch.cuda.synchronize()
    for d in range(2):
        assert not torch.isnan(shifted[d]).any()
        assert torch.equal(plain[d], shifted[d]), d


# ------------------------------------------------------------------------------- model

def _train_step(E, h, dt, train, yprev, monkeypatch):
    """One forward + backward of the two-tower model; returns outputs, loss, gradients and the
    GRU entry points that ran."""
    B, T = 256, 64
    torch.manual_seed(21)
    m = tta.EnhancedTwoTowerModel(E, h).to(DEV).set_compute_dtype(dt)
    m = m.train() if train else m.eval()
    g = torch.Generator().manual_seed(22)
    q = torch.randn(B, T, E, generator=g).to(DEV)
    d = torch.randn(B, T, E, generator=g).to(DEV)
    ran = []
    real = towers.call

    def spy(name, *args):
        if name.startswith("tt_gru_"):
            ran.append(name)
        return real(name, *args)
    monkeypatch.setattr(towers, "call", spy)
    with options(gru_fwd_xc=2, gru_yprev=yprev):
        torch.manual_seed(23)  # the dropout seeds
        qv, dv = m(q, d)
        loss = tta.InfoNCELoss(compute_dtype=dt)(qv, dv)
        loss.backward()
        torch.cuda.synchronize()
    monkeypatch.setattr(towers, "call", real)
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    return qv.detach().clone(), dv.detach().clone(), loss.detach().clone(), grads, ran


def _same_step(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "outputs"
    assert torch.equal(a[2], b[2]), "loss"
    assert len(a[3]) == 44 and a[3].keys() == b[3].keys()
    for k in a[3]:
        assert torch.isfinite(a[3][k]).all(), k
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("E,h", [(16, 128), (300, 256)])
def test_training_step_is_bit_identical_with_dropout(E, h, monkeypatch):
    """Dropout 0.1: both layers run in the previous-state layout."""
    on = _train_step(E, h, BF16, True, 1, monkeypatch)
    off = _train_step(E, h, BF16, True, 0, monkeypatch)
    _same_step(on, off)
    assert on[4].count("tt_gru_fwd_yprev") == 2 and on[4].count("tt_gru_bwd_yprev") == 2 and "tt_gru_fwd" not in on[4]
    assert off[4].count("tt_gru_fwd") == 2 and off[4].count("tt_gru_bwd") == 2
    assert not any(n.endswith("_yprev") for n in off[4])


def test_training_step_is_bit_identical_without_dropout(monkeypatch):
    """drop_p = 0 with gradients: layer 0's Y is layer 1's input and stays as it is; layer 1 runs
    in the previous-state layout."""
    on = _train_step(64, 128, BF16, False, 1, monkeypatch)
    off = _train_step(64, 128, BF16, False, 0, monkeypatch)
    _same_step(on, off)
    assert on[4].count("tt_gru_fwd_yprev") == 1 and on[4].count("tt_gru_fwd") == 1
    assert on[4].count("tt_gru_bwd_yprev") == 1 and on[4].count("tt_gru_bwd") == 1
    assert not any(n.endswith("_yprev") for n in off[4])


@pytest.mark.parametrize("dt,h", [(torch.float32, 128), (BF16, 64)])
def test_unsupported_shapes_run_the_default_layout(dt, h, monkeypatch):
    """fp32, and bf16 at H 128 (not a column-split width): the query says no, the step runs tt_gru_fwd / tt_gru_bwd and matches."""
    on = _train_step(16, h, dt, True, 1, monkeypatch)
    off = _train_step(16, h, dt, True, 0, monkeypatch)
    _same_step(on, off)
    assert not any(n.endswith("_yprev") for n in on[4]) and on[4].count("tt_gru_fwd") == 2
