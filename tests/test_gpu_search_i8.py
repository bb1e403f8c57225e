"""Int8 document index: tt_quantize_rows_i8, tt_search_topk_i8 (fused scan, int8 MFMA score
block + column-split top-k, score block + radix selection), tt_gather_scores and
SearchIndex(score_dtype=torch.int8, rescore=...).

Integer dot products are exact and the two scale multiplies are single fp32 roundings in a
fixed order, so the quantisation and every search form are compared bit for bit with a
restatement in torch on the CPU. The end-to-end test plants documents whose cosine margin over
every other document exceeds twice the worst-case quantisation error at h 64 (0.064, DESIGN.md
"Int8 index"), so the int8 top-5 set must equal the fp32 index's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from two_towers_amd import _lib, ops  # noqa: E402
from two_towers_amd._lib import TTError, call, stream_ptr  # noqa: E402

DEV = "cuda"
FLT_MAX = float(np.finfo(np.float32).max)


# ------------------------------------------------------------------ quantisation
def quant_ref(x):
    """The rule of include/tt_hip.h in fp32 on the CPU (tensor divisors: true fp32 divisions)."""
    amax = x.abs().amax(dim=1)
    c127 = torch.full_like(amax, 127.0)
    inv = torch.where(amax > 0, c127 / amax, torch.zeros_like(amax))
    codes = torch.round(x * inv[:, None]).clamp(-127, 127).to(torch.int8)
    return codes, amax / c127


def quant_input(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.rand(rows, 1, generator=g).mul(4).exp()
    x[0] = 0.0  # all-zero row
    if rows > 1:
        x[1] = 0.0
        x[1, cols // 2] = -0.37  # one non-zero entry
    if rows > 2:
        x[2, 3] = -x[2].abs().max() * 1.5  # the largest entry is negative
    if rows > 3:  # amax 127 and n + 0.5 entries: the scale is exactly 1, codes round half to even
        x[3] = (torch.arange(cols) % 100).float() + 0.5
        x[3, ::2] *= -1
        x[3, 5] = 127.0
    return x


@pytest.mark.parametrize("rows,cols,pad", [(1, 16, 0), (7, 64, 0), (300, 512, 0), (5, 1024, 0), (7, 64, 8)])
def test_quantize_rows_bit_exact(rows, cols, pad):
    x = quant_input(rows, cols, 100 + rows + cols)
    xd = torch.zeros(rows, cols + pad).to(DEV)
    xd[:, :cols] = x.to(DEV)
    codes, scale = ops.quantize_rows_i8(xd[:, :cols])  # pad > 0: ld > cols
    rc, rs = quant_ref(x)
    assert codes.dtype == torch.int8 and tuple(codes.shape) == (rows, cols) and scale.dtype == torch.float32
    assert torch.equal(codes.cpu(), rc)
    assert torch.equal(scale.cpu(), rs)
    assert int(codes[0].abs().max()) == 0 and float(scale[0]) == 0.0
    if rows > 3:
        assert float(scale[3]) == 1.0
        assert codes[3, :6].cpu().tolist() == [0, 2, -2, 4, -4, 127]  # -0.5 1.5 -2.5 3.5 -4.5 | 127


def test_quantize_zero_rows_is_a_noop():
    codes, scale = ops.quantize_rows_i8(torch.empty(0, 64, device=DEV))
    assert tuple(codes.shape) == (0, 64) and scale.numel() == 0


# ------------------------------------------------------------------ search
def search_case(Q, N, h, seed, extreme=False):
    g = torch.Generator().manual_seed(seed)
    qc = torch.randint(-127, 128, (Q, h), generator=g, dtype=torch.int8)
    dc = torch.randint(-127, 128, (N, h), generator=g, dtype=torch.int8)
    qs = torch.rand(Q, generator=g) * 0.01 + 1e-3
    ds = torch.rand(N, generator=g) * 0.01 + 1e-3
    a, b = N // 3, N - 2  # duplicate documents: equal scores, the lower index first
    dc[b], ds[b] = dc[a], ds[a]
    dc[N // 2 + 1], ds[N // 2 + 1] = dc[5], ds[5]
    if extreme:  # the dot reaches +-127^2 h
        qc[0] = 127
        dc[7] = 127
        dc[8] = -127
    return qc, qs, dc, ds


def search_ref(qc, qs, dc, ds, k):
    dot = qc.long() @ dc.long().T
    s = (dot.to(torch.float32) * ds[None, :]) * qs[:, None]
    val, idx = torch.sort(s, dim=1, descending=True, stable=True)
    return idx[:, :k].to(torch.int32), val[:, :k].contiguous()


def run_search(qc, qs, dc, ds, k):
    idx, val = ops.search_topk_i8(qc.to(DEV), qs.to(DEV), dc.to(DEV), ds.to(DEV), k)
    return idx.cpu(), val.cpu()


SCAN = [(1, 3000, 64, 3), (5, 1025, 128, 1), (64, 4100, 32, 16), (9, 777, 512, 5), (3, 2100, 1024, 4)]
MFMA = [(70, 9000, 64, 3), (130, 5000, 96, 16), (65, 1000, 16, 16)]
SELECT = [(4, 3000, 64, 100), (70, 2500, 128, 1024)]


# qb 0: the default dispatch (the scan only where one pass holds the queries); qb 8: the fused
# scan for every Q <= 64, in groups of up to 8 (k <= 4) / 2 queries
@pytest.mark.parametrize("Q,N,h,k,qb", [c + (0,) for c in SCAN + MFMA + SELECT] + [c + (8,) for c in SCAN])
def test_search_bit_exact(Q, N, h, k, qb):
    qc, qs, dc, ds = search_case(Q, N, h, seed=Q * 7 + h, extreme=(h == 1024))
    with _lib.option("search_i8_qb", qb):
        idx, val = run_search(qc, qs, dc, ds, k)
    ridx, rval = search_ref(qc, qs, dc, ds, k)
    if h == 1024:
        assert int((qc[0].long() * dc[7].long()).sum()) == 127 * 127 * 1024
    assert torch.equal(idx, ridx)
    assert torch.equal(val, rval)


@pytest.mark.parametrize("qb", [1, 4, 16])
def test_scan_group_sizes_return_the_same_bits(qb):
    """Option search_i8_qb > 0 takes the scan up to 64 queries and caps the queries per pass; a
    last group that is not full (Q 13) scores its spare slots and must leave them out."""
    qc, qs, dc, ds = search_case(13, 2500, 64, seed=qb)
    for k in (3, 9):
        with _lib.option("search_i8_qb", qb):
            idx, val = run_search(qc, qs, dc, ds, k)
        ridx, rval = search_ref(qc, qs, dc, ds, k)
        assert torch.equal(idx, ridx) and torch.equal(val, rval)


def test_prefix_property_across_forms():
    qc, qs, dc, ds = search_case(70, 3000, 64, seed=11)
    # 65 queries take the MFMA score block; their first 64 alone the block as well by default,
    # the fused scan with the option; a query's row is the same in all three
    i65, v65 = run_search(qc[:65], qs[:65], dc, ds, 16)
    for qb in (0, 2):
        with _lib.option("search_i8_qb", qb):
            i64, v64 = run_search(qc[:64], qs[:64], dc, ds, 16)
        assert torch.equal(i65[:64], i64) and torch.equal(v65[:64], v64)
    for Q, qb in ((2, 0), (4, 2), (70, 0)):  # scan (one pass, two passes) / split top-k against the selection
        with _lib.option("search_i8_qb", qb):
            i16, v16 = run_search(qc[:Q], qs[:Q], dc, ds, 16)
        i100, v100 = run_search(qc[:Q], qs[:Q], dc, ds, 100)
        assert torch.equal(i100[:, :16], i16) and torch.equal(v100[:, :16], v16)
        i3, v3 = run_search(qc[:Q], qs[:Q], dc, ds, 3)
        assert torch.equal(i100[:, :3], i3) and torch.equal(v100[:, :3], v3)


# ------------------------------------------------------------------ gather scores
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_gather_scores_exact(dt):
    g = torch.Generator().manual_seed(3)
    N = 500
    for h in (64, 512):
        d = torch.randint(-3, 4, (N, h), generator=g).float()
        dd = d.to(DEV).to(dt)
        for Q in (3, 70):
            q = torch.randint(-3, 4, (Q, h), generator=g).float()
            for R in (1, 40, 1024):
                cand = torch.randint(0, N, (Q, R), generator=g, dtype=torch.int32)
                bad = (Q - 1, R // 2)
                cand[bad] = N if R != 40 else -1  # one candidate out of range
                out = ops.gather_scores(q.to(DEV), dd, cand.to(DEV)).cpu()
                ref = (q.double()[:, None, :] * d.double()[cand.clamp(0, N - 1).long()]).sum(-1)
                ref[bad] = -FLT_MAX
                assert out.dtype == torch.float32 and torch.equal(out.double(), ref), (h, Q, R)


# ------------------------------------------------------------------ SearchIndex
def planted_corpus(seed=0, h=64, N=4096, nq=8, plant=5):
    g = torch.Generator().manual_seed(seed)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)  # noqa: E731
    docs = unit(torch.randn(N, h, generator=g))
    q = unit(torch.randn(nq, h, generator=g))
    where = torch.randperm(N, generator=g)[:nq * plant].reshape(nq, plant)
    for i in range(nq):
        docs[where[i]] = unit(q[i] + 0.3 * unit(torch.randn(plant, h, generator=g)))
    cos = unit(q.double()) @ unit(docs.double()).T
    return q, docs, where, cos


@pytest.fixture(scope="module")
def indexes():
    from two_towers_amd.data import Vocab
    from two_towers_amd.margin import TwoTowerModel
    from two_towers_amd.serving import SearchIndex
    q, docs, where, cos = planted_corpus()
    N, h = docs.shape
    words = [f"t{i}" for i in range(50)]
    texts = [f"t{i % 50} t{(i * 7) % 50} doc{i}" for i in range(N)]
    vocab = Vocab(words, np.random.default_rng(1).standard_normal((50, 24)).astype(np.float32))
    torch.manual_seed(2)
    m = TwoTowerModel(24, h).to(DEV).eval()
    mk = lambda **kw: SearchIndex(m, vocab, texts, doc_vectors=docs, **kw)  # noqa: E731
    return {"q": q, "docs": docs, "where": where, "cos": cos, "texts": texts,
            "f32": mk(), "i8": mk(score_dtype=torch.int8), "i8r": mk(score_dtype=torch.int8, rescore=4),
            "i8host": mk(score_dtype=torch.int8, keep_vectors=False)}


def test_index_precondition_and_int8_top5_set(indexes):
    cos, where = indexes["cos"], indexes["where"]
    nq, plant = where.shape
    for i in range(nq):
        planted = cos[i, where[i]].sort(descending=True).values
        others = cos[i].clone()
        others[where[i]] = -2.0
        # twice the worst-case int8 error at h 64, and planted scores that fp32 can order
        assert float(planted[-1] - others.max()) > 0.13
        assert float((planted[:-1] - planted[1:]).min()) > 1e-5
    qd = indexes["q"].to(DEV)
    fi, fv = indexes["f32"].topk(qd, 5)
    ref_order = torch.stack([where[i][cos[i, where[i]].argsort(descending=True)] for i in range(nq)])
    assert torch.equal(fi.cpu(), ref_order)
    ii, iv = indexes["i8"].topk(qd, 5)
    assert ii.dtype == torch.int64 and iv.dtype == torch.float32
    assert torch.equal(ii.cpu().sort(dim=1).values, fi.cpu().sort(dim=1).values)
    assert float((iv.cpu().double() - cos.gather(1, ii.cpu())).abs().max()) < 0.064
    # rescored: the fp32 index's order, and the exact cosines
    ri, rv = indexes["i8r"].topk(qd, 5)
    assert torch.equal(ri.cpu(), fi.cpu())
    assert float((rv.cpu().double() - cos.gather(1, ri.cpu())).abs().max()) < 1e-6


def test_index_layout_and_host_vectors(indexes, tmp_path):
    from two_towers_amd.serving import SearchIndex
    i8, i8r, i8host = indexes["i8"], indexes["i8r"], indexes["i8host"]
    N, h = indexes["docs"].shape
    assert i8.doc_normed is None and i8.doc_codes.dtype == torch.int8 and tuple(i8.doc_codes.shape) == (N, h)
    assert i8.doc_scales.dtype == torch.float32 and tuple(i8.doc_scales.shape) == (N,)
    assert i8r.doc_normed.dtype == torch.float32
    rc, rs = quant_ref(i8r.doc_normed.cpu())
    for ix in (i8, i8r, i8host):
        assert torch.equal(ix.doc_codes.cpu(), rc) and torch.equal(ix.doc_scales.cpu(), rs)
    assert i8.doc_vectors.device.type == "cuda" and i8host.doc_vectors.device.type == "cpu"
    path = str(tmp_path / "doc_embeddings.pt")
    i8host.save(path)
    assert torch.equal(SearchIndex.load_vectors(path), indexes["docs"])
    a = i8host.topk(indexes["q"].to(DEV), 5)
    b = i8.topk(indexes["q"].to(DEV), 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_index_search_response_and_rescore_clamp(indexes):
    for name in ("i8", "i8r"):
        res = indexes[name].search("t3 t21", top_k=3)
        assert res["query"] == "t3 t21" and [r["rank"] for r in res["results"]] == [1, 2, 3]
        for r in res["results"]:
            assert set(r) == {"text", "score", "is_ground_truth", "rank"} and isinstance(r["text"], str)
        scores = [r["score"] for r in res["results"]]
        assert scores == sorted(scores, reverse=True)
    # r * k above tt_topk_max() is clamped: 4 * 300 -> a shortlist of 1024
    qd = indexes["q"].to(DEV)
    ri, rv = indexes["i8r"].topk(qd, 300)
    assert tuple(ri.shape) == (8, 300) and torch.equal(ri[:, :5].cpu(), indexes["f32"].topk(qd, 5)[0].cpu())
    assert bool((rv[:, :-1] >= rv[:, 1:]).all())


def test_topk_cosine_int8(indexes):
    from two_towers_amd.retrieval import topk_cosine
    qd, dd = indexes["q"].to(DEV), indexes["docs"].to(DEV)
    idx, val = topk_cosine(qd, dd, k=5, compute_dtype=torch.int8)
    ii, iv = indexes["i8"].topk(qd, 5)
    assert torch.equal(idx, ii) and torch.equal(val, iv)


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_name_the_limit():
    def go(Q, N, h, k, shift=0):
        qc = torch.zeros(Q * h + 16, dtype=torch.int8, device=DEV)
        dc = torch.zeros(N * h + 16, dtype=torch.int8, device=DEV)
        qs, ds = torch.ones(Q, device=DEV), torch.ones(N, device=DEV)
        idx = torch.empty(Q, max(k, 1), dtype=torch.int32, device=DEV)
        val = torch.empty(Q, max(k, 1), dtype=torch.float32, device=DEV)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        call("tt_search_topk_i8", qc.data_ptr(), qs.data_ptr(), Q, dc.data_ptr() + shift, ds.data_ptr(), N, h, k,
             idx.data_ptr(), val.data_ptr(), ws.data_ptr(), stream_ptr(qc.device))

    go(2, 40, 32, 3)  # the well-formed call passes
    with pytest.raises(TTError, match="multiple of 16"):
        go(2, 40, 24, 3)
    with pytest.raises(TTError, match="at most 1024"):
        go(2, 40, 1040, 3)
    with pytest.raises(TTError, match=r"min\(1024, N=40\)"):
        go(2, 40, 32, 41)
    with pytest.raises(TTError, match=r"k=1025 .*min\(1024"):
        go(2, 2000, 32, 1025)
    with pytest.raises(TTError, match="16-byte aligned"):
        go(2, 40, 32, 3, shift=1)
    x = torch.zeros(4, 24, device=DEV)
    with pytest.raises(TTError, match="multiple of 16"):
        ops.quantize_rows_i8(x)
    with pytest.raises(TTError, match="at most 1024"):
        ops.quantize_rows_i8(torch.zeros(2, 1040, device=DEV))
    with pytest.raises(TTError, match="R=1025"):
        ops.gather_scores(torch.zeros(2, 64, device=DEV), torch.zeros(9, 64, device=DEV),
                          torch.zeros(2, 1025, dtype=torch.int32, device=DEV))
