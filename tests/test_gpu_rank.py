"""Full ranks (validate_margin.py:11-54 without a cutoff): tt_rank_best_relevant and
tt_rank_count through the C ABI, and first_relevant_rank / validate_full_rank on top.

bf16 with h in {128, 256, 512} runs the streamed scan of tt_score.hip with the counting
epilogue; other shapes (and option rank_gemm = 1) store a row block of scores through tt_gemm
and count over it. Integer-valued operands in [-3, 3] make every dot product exact in fp32
and bf16 whatever the summation order, so ranks, thresholds and threshold columns are
compared exactly with a float64 reference of the rule: stable sort by (-score, index),
position of the first relevant column."""
import os
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import two_towers_amd as tta  # noqa: E402
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import call, dtype_code, option  # noqa: E402
from two_towers_amd.retrieval import topk_cosine  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"


def ref_ranks(q, d, relevant):
    """(rank, theta, tcol) per query from a stable float64 sort by (-score, index)."""
    s = q.double().to(DEV) @ d.double().to(DEV).t()
    order = torch.sort(-s, dim=1, stable=True).indices.cpu()
    s = s.cpu()
    pos = torch.empty_like(order)
    pos.scatter_(1, order, torch.arange(order.shape[1]).repeat(order.shape[0], 1))
    rank, theta, tcol = [], [], []
    for i, rel in enumerate(relevant):
        if not rel:
            rank.append(0), theta.append(0.0), tcol.append(-1)
            continue
        p = int(pos[i, sorted(rel)].min())
        t = int(order[i, p])
        rank.append(p + 1), theta.append(float(s[i, t])), tcol.append(t)
    return (torch.tensor(rank, dtype=torch.int32), torch.tensor(theta, dtype=torch.float64),
            torch.tensor(tcol, dtype=torch.int32))


def run_rank(q, d, relevant, dt, blocks=None, garbage=False):
    """The two C entries; blocks: consecutive document block sizes counted with col_offset
    and accumulate. Returns (rank, theta, tcol, count) on the host."""
    lib = _lib.load()
    Q, h = q.shape
    N = d.shape[0]
    qd, dd = q.to(DEV, dt).contiguous(), d.to(DEV, dt).contiguous()
    ptr, idx = tta.relevance_csr(relevant)
    ptr, idx = ptr.to(DEV), idx.to(DEV)
    theta = torch.full((Q,), 7.0, dtype=torch.float32, device=DEV)
    tcol = torch.full((Q,), 12345, dtype=torch.int32, device=DEV)
    count = torch.full((Q,), 0x7F7F7F7F if garbage else 0, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call("tt_rank_best_relevant", dtype_code(dt), qd.data_ptr(), Q, dd.data_ptr(), N, h, ptr.data_ptr(),
         idx.data_ptr(), theta.data_ptr(), tcol.data_ptr(), None, st)
    b0 = 0
    for n in blocks or [N]:
        # the workspace's previous contents must not matter
        ws = torch.full((max(lib.tt_rank_count_ws_size(dtype_code(dt), Q, n, h), 1),), 0x7F, dtype=torch.uint8,
                        device=DEV)
        call("tt_rank_count", dtype_code(dt), qd.data_ptr(), Q, dd[b0:].data_ptr(), n, h, b0, theta.data_ptr(),
             tcol.data_ptr(), count.data_ptr(), 1 if b0 else 0, ws.data_ptr(), st)
        b0 += n
    assert b0 == N
    torch.cuda.synchronize()
    tc = tcol.cpu()
    cnt = count.cpu()
    return torch.where(tc >= 0, cnt + 1, torch.zeros_like(cnt)), theta.cpu(), tc, cnt


def make_case(Q, N, h, seed):
    """Integer-valued rows, planted duplicates, and the relevance mix: three documents of
    which two are exact duplicates, empty rows, single documents, the last column (in the
    last, partial chunk), a duplicate of a lower-indexed irrelevant document, two singles."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-3, 4, (Q, h), generator=g).float()
    d = torch.randint(-3, 4, (N, h), generator=g).float()
    a, b = 3, N // 2            # relevant twins: the best relevant ties between two columns
    lo, hi = 5, N - 2           # hi is relevant, its lower-indexed twin lo is not: lo beats hi
    d[b] = d[a]
    d[hi] = d[lo]
    relevant = []
    for i in range(Q):
        r = int(torch.randint(0, N, (1,), generator=g))
        kind = i % 6
        relevant.append([{a, b, r}, set(), {r}, {N - 1}, {hi}, {r, N - 1}][kind])
    return q, d, relevant


def check_exact(q, d, relevant, dt, **kw):
    rr, rth, rtc = ref_ranks(q, d, relevant)
    rank, theta, tcol, _ = run_rank(q, d, relevant, dt, **kw)
    assert torch.equal(tcol, rtc)
    assert torch.equal(theta.double(), rth)
    assert torch.equal(rank, rr), (rank - rr).abs().max()
    return rank


CASES = [  # Q, N, h
    (300, 1000, 256),    # partial last tile
    (513, 513, 256),     # one row past a 512-row workgroup; Q = N
    (129, 4100, 512),    # 4-wave scan, 65 splits of one tile each (RT 2, tps 1)
    (40, 70, 128),       # two chunks
    (96, 640, 64),       # stored path
    (33, 999, 96),       # stored path
    (1, 64, 128),
]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Q,N,h", CASES)
def test_rank_exact(dt, Q, N, h):
    q, d, relevant = make_case(Q, N, h, Q * 7919 + N * 31 + h)
    rank = check_exact(q, d, relevant, dt)
    lo_hi = [i for i in range(Q) if i % 6 == 4]
    if lo_hi:  # the relevant twin never ranks first: its irrelevant lower-indexed twin beats it
        assert int(rank[lo_hi].min()) >= 2


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Q,N,h", [(40, 70, 128), (300, 1000, 256)])
def test_rank_negative_thresholds(dt, Q, N, h):
    """Every query's best relevant score is negative and N is no multiple of 64: the zero
    columns that pad the last tile would beat it, and must not be counted."""
    g = torch.Generator().manual_seed(Q + N)
    q = torch.randint(-3, 4, (Q, h), generator=g).float()
    d = torch.randint(-3, 4, (N, h), generator=g).float()
    d[N - 1] = -q[0]                       # the most negative score there is, in the partial tile
    s = q.double() @ d.double().t()
    relevant = []
    for i in range(Q):
        neg = torch.nonzero(s[i] < 0).flatten()
        relevant.append({int(neg[int(torch.randint(0, len(neg), (1,), generator=g))])})
    relevant[0] = {N - 1}
    rr, rth, _ = ref_ranks(q, d, relevant)
    assert bool((rth < 0).all()) and int(rr[0]) == N
    rank = check_exact(q, d, relevant, dt)
    assert int(rank.max()) <= N


@pytest.mark.parametrize("h", [128, 256, 512])
def test_rank_all_scores_equal(h):
    """Every score equal: only the column decides, rank = tcol + 1."""
    Q, N = 70, 900
    q, d = torch.ones(Q, h), torch.ones(N, h)
    relevant = [{(i * 13) % N, N - 1 - i} for i in range(Q)]
    rank, theta, tcol, _ = run_rank(q, d, relevant, torch.bfloat16)
    assert torch.equal(tcol, torch.tensor([min(r) for r in relevant], dtype=torch.int32))
    assert torch.equal(rank, tcol + 1)
    assert bool((theta == float(h)).all())


@pytest.mark.parametrize("gemm", [0, 1])
def test_rank_blocks_accumulate_to_the_whole(gemm):
    """(300, 4100, 256) counted in one call equals the same in blocks of 1000, 1000 and 2100
    with col_offset and accumulate; accumulate = 0 overwrites a count buffer of garbage."""
    q, d, relevant = make_case(300, 4100, 256, 99)
    with option("rank_gemm", gemm):
        whole = check_exact(q, d, relevant, torch.bfloat16, garbage=True)
        parts = check_exact(q, d, relevant, torch.bfloat16, blocks=[1000, 1000, 2100], garbage=True)
    assert torch.equal(whole, parts)


def test_first_relevant_rank_doc_block_and_csr_input():
    q, d, relevant = make_case(300, 4100, 256, 98)
    rr, _, _ = ref_ranks(q, d, relevant)
    # integer rows: their cosines are no longer exact, so compare the calls with each other
    qd, dd = q.to(DEV), d.to(DEV)
    whole = tta.first_relevant_rank(qd, dd, relevant, compute_dtype=torch.bfloat16)
    assert whole.dtype == torch.int32 and whole.shape == (300,)
    blocked = tta.first_relevant_rank(qd, dd, relevant, compute_dtype=torch.bfloat16, doc_block=1000)
    assert torch.equal(whole, blocked)
    csr = tta.first_relevant_rank(qd, dd, tta.relevance_csr(relevant), compute_dtype=torch.bfloat16, doc_block=1000)
    assert torch.equal(whole, csr)
    assert torch.equal(whole == 0, (rr == 0).to(DEV))
    f32 = tta.first_relevant_rank(qd, dd, relevant, doc_block=2050)
    assert torch.equal(f32, tta.first_relevant_rank(qd, dd, relevant))
    with pytest.raises(_lib.TTError, match="outside"):
        tta.first_relevant_rank(qd, dd, [{4100}] + [set()] * 299)
    assert tta.first_relevant_rank(qd[:0], dd, []).shape == (0,)


@pytest.mark.parametrize("Q,N,h", [(1000, 3000, 256), (300, 4100, 128), (1000, 3000, 512)])
def test_rank_scan_matches_stored_path(Q, N, h):
    """Random (non-integer) normalised bf16 rows: the streamed count and the stored path form
    every score, thresholds included, with the same MFMA instruction and k order, so ranks,
    theta and tcol agree bit for bit -- a threshold one ulp off would move document tcol
    itself, or a near-tie, to the other side. The ranks also equal the ones read off the
    exact top-k wherever the relevant document lies inside it."""
    g = torch.Generator().manual_seed(Q + N + h)
    q = torch.nn.functional.normalize(torch.randn(Q, h, generator=g), dim=1)
    d = torch.nn.functional.normalize(torch.randn(N, h, generator=g), dim=1)
    d[N - 7] = d[11]
    relevant = [set(torch.randint(0, N, (i % 4,), generator=g).tolist()) | ({11, N - 7} if i % 5 == 0 else set())
                for i in range(Q)]
    srank, sth, stc, _ = run_rank(q, d, relevant, torch.bfloat16)
    with option("rank_gemm", 1):
        grank, gth, gtc, _ = run_rank(q, d, relevant, torch.bfloat16)
    assert torch.equal(stc, gtc)
    assert torch.equal(sth.view(torch.int32), gth.view(torch.int32))
    assert torch.equal(srank, grank)
    # against float64 on the bf16-rounded rows: the threshold is the best relevant score
    rr, rth, _ = ref_ranks(q.bfloat16().float(), d.bfloat16().float(), relevant)
    assert float((sth.double() - rth).abs().max()) < 1e-5
    assert torch.equal(srank == 0, rr == 0)

    k = min(1024, N)
    qd, dd = q.to(DEV), d.to(DEV)
    ranks = tta.first_relevant_rank(qd, dd, relevant, compute_dtype=torch.bfloat16).cpu()
    top = topk_cosine(qd, dd, k=k, compute_dtype=torch.bfloat16)[0].cpu().tolist()
    seen = 0
    for i, (row, rel) in enumerate(zip(top, relevant)):
        first = next((p for p, j in enumerate(row, 1) if j in rel), None)
        if first is not None:
            assert int(ranks[i]) == first, (i, int(ranks[i]), first)
            seen += 1
        else:
            assert int(ranks[i]) == 0 or int(ranks[i]) > k
    assert seen > Q // 4


# ---------------------------------------------------------------- the reference's numbers
def golden():
    z = np.load(os.path.join(GOLD, "fullrank_tiny.npz"), allow_pickle=False)
    m = tta.TwoTowerModel(16, 8)
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")})
    vocab = tta.Vocab([str(w) for w in z["words"]], z["vecs"])
    m = m.to(DEV).eval().set_embedding_table(vocab.device_table(DEV))
    docs = [str(t) for t in z["docs"]]
    queries = [str(t) for t in z["queries"]]
    ptr, idx = z["rel_ptr"].tolist(), z["rel_idx"].tolist()
    relevant = [set(idx[ptr[i]:ptr[i + 1]]) for i in range(len(queries))]
    return z, m, vocab, queries, docs, relevant


def test_full_rank_matches_reference_compute_mrr():
    """validate_margin.compute_mrr run by the reference on the CPU (tools/gen_fullrank_golden.py):
    the same integer rank, hence the same reciprocal rank, for every query -- those without
    relevant documents score 0 -- and the same first three documents."""
    z, m, vocab, queries, docs, relevant = golden()
    assert sorted({len(r) for r in relevant}) == [0, 1, 3]
    out = tta.validate_full_rank(m, vocab, queries, docs, relevant, num_queries=len(queries))
    valid = [i for i, r in enumerate(relevant) if r]
    assert out["query_index"] == valid
    assert out["rank"] == z["rank"][valid].tolist()
    assert out["reciprocal_rank"] == z["rr"][valid].tolist()
    assert out["top3"] == z["top3"][valid].tolist()
    assert out["mrr"] == pytest.approx(float(z["rr"][valid].mean()), abs=1e-12)
    assert np.abs(np.array(out["top3_scores"]) - z["top3_scores"][valid]).max() < 1e-4
    # every query, the empty ones included, straight through first_relevant_rank
    from two_towers_amd.retrieval import _tokenizer_of, encode_texts
    tok = _tokenizer_of(m)
    qv = encode_texts(m, queries, vocab, "query", tokenize=tok)
    dv = encode_texts(m, docs, vocab, "doc", tokenize=tok)
    ranks = tta.first_relevant_rank(qv, dv, relevant).cpu()
    assert ranks.tolist() == z["rank"].tolist()
    rr = [1.0 / r if r else 0.0 for r in ranks.tolist()]
    assert rr == z["rr"].tolist()
    assert tta.mrr_from_ranks(ranks) == pytest.approx(float(z["rr"].mean()), abs=1e-12)


def test_validate_full_rank_samples_and_writes_the_reference_format(tmp_path):
    z, m, vocab, queries, docs, relevant = golden()
    path = str(tmp_path / "validation_results.txt")
    out = tta.validate_full_rank(m, vocab, queries, docs, relevant, num_queries=5, seed=7, out_path=path)
    valid = [i for i, r in enumerate(relevant) if r]
    assert out["query_index"] == random.Random(7).sample(valid, 5)
    assert out["rank"] == z["rank"][out["query_index"]].tolist()
    text = open(path, encoding="utf-8").read()
    blocks = text.split("\nQuery: ")[1:]
    assert len(blocks) == 5 and text.startswith("\nQuery: ")
    for i, rr, top, blk in zip(out["query_index"], out["reciprocal_rank"], out["top3"], blocks):
        lines = blk.split("\n")
        truth = docs[min(relevant[i])]
        assert lines[0] == queries[i]
        assert lines[1] == f"Ground Truth Answer: {truth}"
        assert lines[2] == f"Ground Truth Passage: {truth}"
        assert lines[3] == f"MRR: {rr:.4f}"
        for n, (j, line) in enumerate(zip(top, lines[4:7]), 1):
            mt = re.fullmatch(r"(\d)\. \[(✓| )\] \((-?\d\.\d{4})\) (.*)\.\.\.", line)
            assert mt and int(mt.group(1)) == n and mt.group(4) == docs[j][:100]
            assert (mt.group(2) == "✓") == (j in relevant[i])
        assert lines[7:] == [""]
    # appended, not overwritten
    tta.validate_full_rank(m, vocab, queries, docs, relevant, num_queries=1, seed=1, out_path=path)
    assert open(path, encoding="utf-8").read().count("\nQuery: ") == 6
