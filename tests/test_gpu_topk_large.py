"""Exact top-k for k in 17..1024: tt_topk_rows (radix select + ordered compaction + bitonic
sort, tt_select.hip) on its own, behind tt_search_topk and tt_hardneg_topk, and through the
Python surface (SearchIndex, retrieval.topk_cosine, HardNegativeMarginLoss).

The selection does no arithmetic, so crafted floats compare exactly; through the two scoring
entry points integer-valued operands make every score exact in fp32 and bf16, so indices --
long tie runs across the k boundary included, which go to the lower column -- and values are
compared bit-exactly against a stable float64 sort."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import two_towers_amd as tta  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from two_towers_amd import _lib, retrieval  # noqa: E402
from two_towers_amd._lib import TTError, call, dtype_code  # noqa: E402

DEV = "cuda"


def stream():
    return torch.cuda.current_stream().cuda_stream


def ws_bytes(n, fill=None):
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    return ws


def ref_sorted(s, lab, k):
    """Stable float64 sort of every row of s (CPU) with column lab + row set to -1."""
    s = s.double().clone()
    if lab >= 0:
        rows = torch.arange(s.shape[0])
        s[rows, lab + rows] = -1.0
    order = torch.sort(-s, dim=1, stable=True).indices[:, :k]
    return order, torch.gather(s, 1, order)


def run_rows(S, k, lab, fill=None):
    lib = _lib.load()
    rows, cols = S.shape
    Sd = S.to(DEV).contiguous()
    idx = torch.empty(rows, k, dtype=torch.int32, device=DEV)
    val = torch.empty(rows, k, dtype=torch.float32, device=DEV)
    ws = ws_bytes(lib.tt_topk_rows_ws_size(rows, cols, k), fill)
    call("tt_topk_rows", Sd.data_ptr(), rows, cols, cols, lab, k, idx.data_ptr(), val.data_ptr(), ws.data_ptr(),
         stream())
    torch.cuda.synchronize()
    return idx.cpu().long(), val.cpu()


def run_search(q, d, k, dt, fill=None):
    lib = _lib.load()
    Q, h = q.shape
    N = d.shape[0]
    qd, dd = q.to(DEV).contiguous(), d.to(DEV, dt).contiguous()
    idx = torch.empty(Q, k, dtype=torch.int32, device=DEV)
    val = torch.empty(Q, k, dtype=torch.float32, device=DEV)
    ws = ws_bytes(lib.tt_search_ws_size(dtype_code(dt), Q, N, h, k), fill)
    call("tt_search_topk", dtype_code(dt), qd.data_ptr(), Q, dd.data_ptr(), N, h, k, idx.data_ptr(), val.data_ptr(),
         ws.data_ptr(), stream())
    torch.cuda.synchronize()
    return idx.cpu().long(), val.cpu()


def run_hardneg(q, d, lab, k, dt, fill=None):
    lib = _lib.load()
    B, h = q.shape
    nd = d.shape[0]
    qd, dd = q.to(DEV, dt).contiguous(), d.to(DEV, dt).contiguous()
    idx = torch.empty(B, k, dtype=torch.int32, device=DEV)
    val = torch.empty(B, k, dtype=torch.float32, device=DEV)
    ws = ws_bytes(lib.tt_hardneg_ws_size(dtype_code(dt), B, nd, h, k), fill)
    call("tt_hardneg_topk", dtype_code(dt), qd.data_ptr(), B, dd.data_ptr(), nd, h, lab, k, idx.data_ptr(),
         val.data_ptr(), ws.data_ptr(), stream())
    torch.cuda.synchronize()
    return idx.cpu().long(), val.cpu()


# ---------------------------------------------------------------- 1. tt_topk_rows, crafted floats
POOL = [0.0, -0.0, float("inf"), float("-inf"), 1e-40, -1e-40, 1.4e-45, -1.0, 1.0, 0.5, -0.5, 0.25, -0.25,
        0.75, -0.75, 0.1, -0.1, 0.3, -0.3, 0.7, -0.7, 0.9, -0.9, 0.999, -0.999, 1.0000001, -1.0000001, 2.0, -2.0,
        3.5, -3.5, 1e-38, -1e-38, 1e30, -1e30, 3.4e38, -3.4e38, 123.456, -123.456, 0.33333334]


def crafted(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor(POOL, dtype=torch.float32)
    assert int((pool.view(torch.int32) == -2 ** 31).sum()) == 1 and float(pool[4]) > 0  # -0.0 and a denormal survive
    return pool[torch.randint(0, len(POOL), (rows, cols), generator=g)]


@pytest.mark.parametrize("rows,cols,k,lab", [(1, 17, 17, -1), (5, 1000, 17, 0), (3, 5000, 1000, -1),
                                             (130, 4100, 100, 7), (2, 20000, 1024, -1), (7, 1025, 1024, 3),
                                             (4, 70000, 256, -1)])
def test_topk_rows_crafted_floats_exact(rows, cols, k, lab):
    S = crafted(rows, cols, rows * 131 + cols + k)
    ri, rv = ref_sorted(S, lab, k)
    gi, gv = run_rows(S, k, lab, fill=0x5A)
    assert torch.equal(gi, ri)
    assert bool((gv.double() == rv).all())


def test_topk_rows_all_equal():
    """Every score equal: the answer is the k lowest unmasked columns, in order."""
    rows, cols, k = 70, 3000, 1000
    S = torch.full((rows, cols), 0.25)
    gi, gv = run_rows(S, k, 0)
    ri, rv = ref_sorted(S, 0, k)
    assert torch.equal(gi, ri)
    assert bool((gv.double() == rv).all())
    for r in (0, 1, 69):
        assert gi[r].tolist() == [c for c in range(k + 1) if c != r]


def test_topk_rows_small_k_and_empty():
    """The entry point takes any 1 <= k, and rows = 0 is a no-op."""
    S = crafted(9, 9000, 3)
    for k in (1, 16):
        gi, gv = run_rows(S, k, 2)
        ri, rv = ref_sorted(S, 2, k)
        assert torch.equal(gi, ri) and bool((gv.double() == rv).all())
    call("tt_topk_rows", None, 0, 100, 100, -1, 20, None, None, None, stream())


# ---------------------------------------------------------------- 2. through tt_search_topk
def search_operands(Q, N, h):
    g = torch.Generator().manual_seed(Q * 1000 + N)
    q = torch.randint(-3, 4, (Q, h), generator=g).float()
    d = torch.randint(-3, 4, (N, h), generator=g).float()
    d[N // 2] = d[N // 3]
    d[N - 1] = d[7]
    return q, d


SEARCH_CASES = [(1, 3000, 64, 17), (5, 1025, 128, 100), (64, 4100, 32, 1000), (70, 9000, 64, 33),
                (130, 5000, 96, 1024)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Q,N,h,k", SEARCH_CASES)
def test_search_topk_large_exact(dt, Q, N, h, k):
    q, d = search_operands(Q, N, h)
    ri, rv = ref_sorted(q.double() @ d.double().t(), -1, k)
    gi, gv = run_search(q, d, k, dt)
    assert torch.equal(gi, ri)
    assert torch.equal(gv.double(), rv)


# ---------------------------------------------------------------- 3. through tt_hardneg_topk
def hardneg_operands(B, nd, h):
    g = torch.Generator().manual_seed(B * 7919 + nd * 31 + h)
    q = torch.randint(-3, 4, (B, h), generator=g).float()
    d = torch.randint(-3, 4, (nd, h), generator=g).float()
    d[nd // 2] = d[nd // 3]
    d[nd - 1] = d[5]
    d[70] = d[129]
    return q, d


HARDNEG_CASES = [(300, 1000, 256, 0, 17), (64, 4096, 256, 1024, 100), (129, 4100, 512, 7, 1000),
                 (96, 640, 64, 0, 64), (33, 999, 96, -1, 999)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,nd,h,lab,k", HARDNEG_CASES)
def test_hardneg_topk_large_exact(dt, B, nd, h, lab, k):
    q, d = hardneg_operands(B, nd, h)
    ri, rv = ref_sorted(q.double() @ d.double().t(), lab, k)
    gi, gv = run_hardneg(q, d, lab, k, dt)
    assert torch.equal(gi, ri)
    assert torch.equal(gv.double(), rv)


# ---------------------------------------------------------------- 4. prefix consistency
@pytest.mark.parametrize("h", [256, 96])
def test_hardneg_k16_is_prefix_of_k64(h):
    """Random normalised bf16 rows: the k = 16 answer (h 256: streamed scan; h 96: GEMM +
    column split) is the first 16 columns of the k = 64 answer (GEMM + radix selection), bit
    for bit: every path forms a bf16 score with the same MFMA sums."""
    B, nd = 1000, 3000
    g = torch.Generator().manual_seed(h)
    q = torch.nn.functional.normalize(torch.randn(B, h, generator=g), dim=1)
    d = torch.nn.functional.normalize(torch.randn(nd, h, generator=g), dim=1)
    si, sv = run_hardneg(q, d, 0, 16, torch.bfloat16)
    li, lv = run_hardneg(q, d, 0, 64, torch.bfloat16)
    assert torch.equal(si, li[:, :16])
    assert torch.equal(sv.view(torch.int32), lv[:, :16].contiguous().view(torch.int32))


def test_search_k16_is_prefix_of_k40():
    Q, N, h = 70, 5000, 96
    g = torch.Generator().manual_seed(40)
    q = torch.nn.functional.normalize(torch.randn(Q, h, generator=g), dim=1)
    d = torch.nn.functional.normalize(torch.randn(N, h, generator=g), dim=1)
    si, sv = run_search(q, d, 16, torch.bfloat16)
    li, lv = run_search(q, d, 40, torch.bfloat16)
    assert torch.equal(si, li[:, :16])
    assert torch.equal(sv.view(torch.int32), lv[:, :16].contiguous().view(torch.int32))


# ---------------------------------------------------------------- 5. determinism
def test_results_do_not_depend_on_workspace_contents():
    Q, N, h, k = SEARCH_CASES[3]
    q, d = search_operands(Q, N, h)
    a = run_search(q, d, k, torch.bfloat16, fill=0x5A)
    b = run_search(q, d, k, torch.bfloat16, fill=0xA5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    B, nd, h, lab, k = HARDNEG_CASES[2]
    q, d = hardneg_operands(B, nd, h)
    a = run_hardneg(q, d, lab, k, torch.float32, fill=0x5A)
    b = run_hardneg(q, d, lab, k, torch.float32, fill=0xA5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    S = crafted(4, 70000, 9)  # three levels of lists in the workspace
    a = run_rows(S, 256, -1, fill=0x5A)
    b = run_rows(S, 256, -1, fill=0xA5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---------------------------------------------------------------- 6. argument errors
@pytest.mark.parametrize("n,k", [(2000, 1025), (20, 21)])
def test_rejects_k_beyond_the_limit(n, k):
    assert _lib.load().tt_topk_max() == 1024
    h = 16
    x = torch.zeros(n, h, device=DEV)
    out = torch.empty(2 * k, dtype=torch.int32, device=DEV)
    ws = ws_bytes(1 << 20)
    with pytest.raises(TTError, match=f"k={k}"):
        call("tt_topk_rows", x.data_ptr(), 1, n, n, -1, k, out.data_ptr(), None, ws.data_ptr(), stream())
    with pytest.raises(TTError, match=f"k={k}"):
        call("tt_search_topk", 0, x.data_ptr(), 1, x.data_ptr(), n, h, k, out.data_ptr(), None, ws.data_ptr(), stream())
    with pytest.raises(TTError, match=f"k={k}"):
        call("tt_hardneg_topk", 0, x.data_ptr(), 1, x.data_ptr(), n, h, -1, k, out.data_ptr(), None, ws.data_ptr(),
             stream())
    with pytest.raises(TTError, match="1024"):
        tta.mine_hard_negatives(x[:2], x, -1, k)


# ---------------------------------------------------------------- 7. Python surface
def check_cosine_topk(idx, val, q, d, k):
    """The pattern of test_hardneg_bench_size_consistent: the values are the float64 cosines of
    the returned columns, non-increasing, the indices distinct, and no other column scores
    above the k-th value."""
    qn = torch.nn.functional.normalize(q.double(), dim=1)
    dn = torch.nn.functional.normalize(d.double(), dim=1)
    s = qn @ dn.t()
    idx, val = idx.cpu(), val.cpu()
    assert idx.shape == (q.shape[0], k) and idx.dtype == torch.int64
    assert float((torch.gather(s, 1, idx) - val.double()).abs().max()) < 1e-5
    assert bool((val[:, :-1] >= val[:, 1:]).all())
    assert all(len(set(r)) == k for r in idx.tolist())
    s.scatter_(1, idx, -2.0)
    assert bool((s.max(dim=1).values <= val[:, -1].double() + 1e-5).all())


def test_topk_cosine_k100():
    Q, N, h, k = 37, 2500, 64, 100
    g = torch.Generator().manual_seed(7)
    q, d = torch.randn(Q, h, generator=g), torch.randn(N, h, generator=g)
    idx, val = retrieval.topk_cosine(q.to(DEV), d.to(DEV), k=k)
    check_cosine_topk(idx, val, q, d, k)


def test_search_index_top50():
    from two_towers_amd.data import Vocab
    from two_towers_amd.margin import TwoTowerModel
    from two_towers_amd.serving import SearchIndex
    E, H, n_docs, k = 24, 32, 400, 50
    rng = np.random.default_rng(5)
    words = [f"t{i}" for i in range(300)]
    docs = [" ".join(words[j] for j in rng.integers(0, len(words), int(rng.integers(3, 40)))) for _ in range(n_docs)]
    vocab = Vocab(words, rng.standard_normal((len(words), E)).astype(np.float32))
    torch.manual_seed(6)
    m = TwoTowerModel(E, H).to(DEV).eval()
    g = torch.Generator().manual_seed(8)
    dv = torch.randn(n_docs, H, generator=g)
    index = SearchIndex(m, vocab, docs, doc_vectors=dv)
    qv = torch.randn(5, H, generator=g)
    idx, val = index.topk(qv.to(DEV), k=k)
    check_cosine_topk(idx, val, qv, dv, k)
    res = index.search(docs[3], top_k=k)["results"]
    assert len(res) == k and [r["rank"] for r in res] == list(range(1, k + 1))
    scores = [r["score"] for r in res]
    assert all(a >= b for a, b in zip(scores, scores[1:]))
    with pytest.raises(ValueError, match="1024"):
        index.search(docs[3], top_k=n_docs + 1)


# ---------------------------------------------------------------- 8. HardNegativeMarginLoss(k=24)
def test_margin_hardneg_fp32_k24():
    """test_margin_hardneg_fp32 at k = 24. Precondition, asserted for all 64 rows: neighbouring
    float64 cosines among a row's first 25 differ by more than 1e-5 (smallest gap 1.48e-5),
    while an fp32 cosine of 16 terms rounds at about 2e-7, so no row's order can flip."""
    B, h, k = 64, 16, 24
    g = torch.Generator().manual_seed(8)
    q = torch.randn(B, h, generator=g)
    d = torch.randn(B, h, generator=g)
    s = torch.nn.functional.normalize(q.double(), dim=1) @ torch.nn.functional.normalize(d.double(), dim=1).t()
    s[torch.arange(B), torch.arange(B)] = -1.0
    top = torch.sort(s, dim=1, descending=True).values[:, :k + 1]
    gaps = (top[:, :-1] - top[:, 1:]).min(dim=1).values
    print("smallest float64 gap among the first 25 per row:", float(gaps.min()))
    assert int((gaps > 1e-5).sum()) == B

    def rel(a, b):
        a, b = a.double().cpu(), b.double().cpu()
        return float((a - b).abs().max() / (b.abs().max() + 1e-12))

    qd, dd = q.clone().to(DEV).requires_grad_(True), d.clone().to(DEV).requires_grad_(True)
    lossf = tta.HardNegativeMarginLoss(k=k, margin=0.2)
    loss = lossf(qd, dd)
    loss.backward()
    qr, dr = q.clone().requires_grad_(True), d.clone().requires_grad_(True)
    rl, ridx = cpu_ref.hardneg_margin(qr, dr, k, 0.2)
    rl.backward()
    assert torch.equal(lossf.last_indices.long().cpu(), ridx)
    assert abs(float(loss) - float(rl)) < 1e-5
    assert rel(qd.grad, qr.grad) < 1e-4 and rel(dd.grad, dr.grad) < 1e-4
