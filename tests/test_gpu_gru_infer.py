"""The inference GRU forward (tt_gru_fwd_infer: no saved pre-activations, the layer output
optional, the final states written directly) against the training forward tt_gru_fwd with
drop_p = 0 on the same inputs, in every kernel family: column-split (gru_fwd_xs /
gru_fwd_xcp), row-owning (gru_fwd_seq) and per-step (gru_fwd_step, bf16 and fp32).

Reference: the recurrence of nn.GRU (enhanced_two_tower.py:17-33, called at :51, :57), whose
final states :53 and :59 concatenate. The inference instances run the same MFMA sequence
along k and the same gate cell as the training ones, so every value is expected
bit-identical: y to Y everywhere, hfinal[:, d*H:(d+1)*H] to Y at t = T-1 (d = 0) or t = 0
(d = 1). hfinal is allocated with one extra row and 8 extra columns of a sentinel, which
must survive the call.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import GruFwdRec, GruInferRec, call, option, stream_ptr  # noqa: E402
from two_towers_amd.towers import gru_fwd_workspace  # noqa: E402

DEV = "cuda"
PAD = 8  # extra hfinal columns (keeps ldf * element size a multiple of 16)


def _inputs(ntow, B, T, H, seed, dt=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    G = [torch.randn(B * T, 6 * H, generator=g, device=DEV).to(dt) for _ in range(ntow)]
    whh = [[(torch.randn(3 * H, H, generator=g, device=DEV) * H ** -0.5).to(dt) for _ in range(2)]
           for _ in range(ntow)]
    bhn = [[torch.randn(H, generator=g, device=DEV) * 0.5 for _ in range(2)] for _ in range(ntow)]
    return G, whh, bhn


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _sentinel(shape, dt):
    return torch.full(shape, -777.0, dtype=dt, device=DEV)


def _workspace(ntow, B, T, H, dt, use_ws):
    return gru_fwd_workspace(2 * ntow, B, T, H, dt, torch.device(DEV)) if use_ws else None


def _ws_args(ws):
    return (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)


def _status(ws):
    return 0 if ws is None else int(ws[:4].view(torch.int32).item())


def _train(ntow, B, T, H, dt, G, whh, bhn, use_ws):
    """tt_gru_fwd with drop_p = 0 under the options in force: the reference Y."""
    BT = B * T
    Y = [torch.empty(BT, 2 * H, dtype=dt, device=DEV) for _ in range(ntow)]
    S = [[torch.empty(BT, 4 * H, dtype=dt, device=DEV) for _ in range(2)] for _ in range(ntow)]
    hs = torch.empty(ntow * 2, 2, B, H, dtype=torch.float32, device=DEV)
    recs = (GruFwdRec * (2 * ntow))()
    for ti in range(ntow):
        for d in range(2):
            r = recs[ti * 2 + d]
            r.g, r.whh, r.bhn = G[ti][:, d * 3 * H:].data_ptr(), whh[ti][d].data_ptr(), bhn[ti][d].data_ptr()
            r.y, r.x1, r.save = Y[ti][:, d * H:].data_ptr(), None, S[ti][d].data_ptr()
            r.hstate, r.dir = hs[ti * 2 + d].data_ptr(), d
    ws = _workspace(ntow, B, T, H, dt, use_ws)
    call("tt_gru_fwd", _lib.dtype_code(dt), recs, 2 * ntow, B, T, H, 6 * H, 2 * H, 0.0, *_ws_args(ws), stream_ptr())
    torch.cuda.synchronize()
    assert _status(ws) == 0
    return Y


def _infer(ntow, B, T, H, dt, G, whh, bhn, use_ws, want_y, want_f):
    """One tt_gru_fwd_infer call. Returns (y or None, padded hfinal buffers or None, ws)."""
    lib = _lib.load()
    BT = B * T
    ldf = 2 * H + PAD
    Y = [_sentinel((BT, 2 * H), dt) for _ in range(ntow)] if want_y else None
    F = [_sentinel((B + 1, ldf), dt) for _ in range(ntow)] if want_f else None
    nb = lib.tt_gru_infer_scratch_size(_lib.dtype_code(dt), B, T, H, int(not want_y))
    scr = torch.empty(2 * ntow, nb, dtype=torch.uint8, device=DEV) if nb > 0 else None
    recs = (GruInferRec * (2 * ntow))()
    for ti in range(ntow):
        for d in range(2):
            r = recs[ti * 2 + d]
            r.g, r.whh, r.bhn = G[ti][:, d * 3 * H:].data_ptr(), whh[ti][d].data_ptr(), bhn[ti][d].data_ptr()
            r.y = Y[ti][:, d * H:].data_ptr() if want_y else None
            r.hfinal = F[ti][:, d * H:].data_ptr() if want_f else None
            r.scratch = scr[ti * 2 + d].data_ptr() if scr is not None else None
            r.dir = d
    ws = _workspace(ntow, B, T, H, dt, use_ws)
    call("tt_gru_fwd_infer", _lib.dtype_code(dt), recs, 2 * ntow, B, T, H, 6 * H, 2 * H, ldf, *_ws_args(ws),
         stream_ptr())
    torch.cuda.synchronize()
    return Y, F, ws


def _check_family(ntow, B, T, H, dt, use_ws, seed, persistent):
    """Modes (a) y only, (b) hfinal only, (c) both, against the training forward run under the
    same options."""
    G, whh, bhn = _inputs(ntow, B, T, H, seed, dt)
    ref = _train(ntow, B, T, H, dt, G, whh, bhn, use_ws)
    want = []
    for ti in range(ntow):
        y = ref[ti].view(B, T, 2 * H)
        want.append(torch.cat([y[:, T - 1, :H], y[:, 0, H:]], 1))
    lib = _lib.load()
    if persistent:
        assert lib.tt_gru_infer_scratch_size(_lib.dtype_code(dt), B, T, H, 1) == 0
    for want_y, want_f in ((True, False), (False, True), (True, True)):
        Y, F, ws = _infer(ntow, B, T, H, dt, G, whh, bhn, use_ws, want_y, want_f)
        if use_ws:
            assert ws is not None and _status(ws) == 0, "a column-split member wait timed out"
            assert lib.tt_gru_fwd_launches_for(_lib.DT_BF16, 2 * ntow, B, T, H, 6 * H, 2 * H) == 1
        for ti in range(ntow):
            if want_y:
                ne = int((_bits(Y[ti]) != _bits(ref[ti])).sum().item())
                print(f"mode y={want_y} f={want_f} tower {ti}: y differs in {ne} of {Y[ti].numel()}")
                assert ne == 0
            if want_f:
                got = F[ti][:B, :2 * H]
                ne = int((_bits(got) != _bits(want[ti])).sum().item())
                print(f"mode y={want_y} f={want_f} tower {ti}: hfinal differs in {ne} of {got.numel()}")
                assert ne == 0
                pad = _bits(_sentinel((1,), dt))[0]
                assert bool((_bits(F[ti][B:]) == pad).all()), "hfinal: the extra row was written"
                assert bool((_bits(F[ti][:, 2 * H:]) == pad).all()), "hfinal: the extra columns were written"


@pytest.mark.parametrize("H,B,T,ntow", [(512, 300, 2, 1), (256, 64, 1, 2), (512, 3000, 5, 2), (512, 70, 3, 2)])
def test_column_split_inference_forward_is_bit_identical(H, B, T, ntow):
    """gru_fwd_xc = 2 forces the column-split kernels: partial 256-row rounds (B 3000 over 8
    groups per recurrence: 256 + 119), groups without rows (B 70, B 64), one tower, T = 1. At
    H 512 both forms run: gru_fwd_xs (1) and gru_fwd_xcp (0). One launch, status word 0."""
    for xs in ((1, 0) if H == 512 else (1,)):
        with option("gru_fwd_xc", 2), option("gru_fwd_xs", xs):
            _check_family(ntow, B, T, H, torch.bfloat16, True, seed=7 * H + B + T + ntow + xs, persistent=True)


@pytest.mark.parametrize("H,B,T,ntow", [(512, 70, 3, 2), (256, 64, 1, 1), (192, 130, 4, 1)])
def test_row_owning_inference_forward_is_bit_identical(H, B, T, ntow):
    """gru_fwd_xc = 0 and no workspace: gru_fwd_seq, fixed (H 512, 256) and runtime (H 192)
    K-tile counts, tail rows in the last 64-row workgroup."""
    with option("gru_fwd_xc", 0):
        assert _lib.load().tt_gru_fwd_launches(_lib.DT_BF16, T, H) == 1
        _check_family(ntow, B, T, H, torch.bfloat16, False, seed=5 * H + B + T, persistent=True)


@pytest.mark.parametrize("dt,H,B,T,ntow", [(torch.bfloat16, 1024, 130, 3, 1), (torch.bfloat16, 512, 300, 2, 2),
                                           (torch.float32, 24, 5, 4, 1), (torch.float32, 64, 129, 3, 2)])
def test_per_step_inference_forward_is_bit_identical(dt, H, B, T, ntow):
    """gru_step = 1: gru_fwd_step, the only kernel at H 1024 and in fp32. Final-only mode
    reads h_{s-1} from the two-slot image in the scratch instead of Y. H 24 is no multiple of
    the 64-unit tile, B 129 / 130 / 300 need two or more batch tiles."""
    with option("gru_step", 1):
        lib = _lib.load()
        esz = 2 if dt == torch.bfloat16 else 4
        assert lib.tt_gru_infer_scratch_size(_lib.dtype_code(dt), B, T, H, 0) == 2 * B * H * 4
        assert lib.tt_gru_infer_scratch_size(_lib.dtype_code(dt), B, T, H, 1) == 2 * B * H * (4 + esz)
        _check_family(ntow, B, T, H, dt, False, seed=3 * H + B + T, persistent=False)


def test_inference_forward_argument_checks():
    """Both outputs NULL, records that disagree and a misaligned ldf are TT_EINVAL (nothing
    is launched); tt_gru_fwd still rejects a NULL save."""
    lib = _lib.load()
    B, T, H, dt = 8, 2, 64, torch.bfloat16
    G, whh, bhn = _inputs(1, B, T, H, 1, dt)
    y = _sentinel((B * T, 2 * H), dt)
    f = _sentinel((B, 2 * H + PAD), dt)

    def recs(ys, fs):
        r = (GruInferRec * 2)()
        for d in range(2):
            r[d].g, r[d].whh, r[d].bhn = G[0][:, d * 3 * H:].data_ptr(), whh[0][d].data_ptr(), bhn[0][d].data_ptr()
            r[d].y = y[:, d * H:].data_ptr() if ys[d] else None
            r[d].hfinal = f[:, d * H:].data_ptr() if fs[d] else None
            r[d].scratch, r[d].dir = None, d
        return r

    def rc(r, ldf):
        return lib.tt_gru_fwd_infer(_lib.DT_BF16, r, 2, B, T, H, 6 * H, 2 * H, ldf, None, 0, stream_ptr())

    ldf = 2 * H + PAD
    assert rc(recs((0, 0), (0, 0)), ldf) == _lib.TT_EINVAL
    assert rc(recs((1, 0), (1, 1)), ldf) == _lib.TT_EINVAL
    assert rc(recs((1, 1), (1, 0)), ldf) == _lib.TT_EINVAL
    assert rc(recs((0, 0), (1, 1)), 2 * H + 4) == _lib.TT_EINVAL  # 264 bytes per row: not 16-byte aligned
    assert rc(recs((1, 1), (1, 1)), 2 * H + 1) == _lib.TT_EINVAL
    torch.cuda.synchronize()
    pad = _bits(_sentinel((1,), dt))[0]
    assert bool((_bits(y) == pad).all()) and bool((_bits(f) == pad).all())
    assert rc(recs((1, 1), (1, 1)), ldf) == 0  # the same records with a valid ldf run
    torch.cuda.synchronize()
    tr = (GruFwdRec * 1)()
    hs = torch.empty(2, B, H, dtype=torch.float32, device=DEV)
    tr[0].g, tr[0].whh, tr[0].bhn = G[0].data_ptr(), whh[0][0].data_ptr(), bhn[0][0].data_ptr()
    tr[0].y, tr[0].x1, tr[0].save, tr[0].hstate, tr[0].dir = y.data_ptr(), None, None, hs.data_ptr(), 0
    assert lib.tt_gru_fwd(_lib.DT_BF16, tr, 1, B, T, H, 6 * H, 2 * H, 0.0, None, 0, stream_ptr()) == _lib.TT_EINVAL
