"""Batched retrieval and MRR@k (the metric of validate_enhanced.py:19-126).

The reference encodes every document in its own forward pass (validate_enhanced.py:
61-71, one EnhancedDataset per text, max_length 30), scores one query at a time with
F.cosine_similarity and takes torch.topk(10) (:73-80), then averages 1/rank of the
first relevant document (:104-110). Here documents and queries are encoded in large
batches through the fused towers, and scoring + top-k is the fused tt_hardneg_topk
kernel (cosine GEMM + per-row top-k) with a stated tie-break: equal scores rank the
lower document index first.

Full ranks (validate_margin.py:11-54, compute_mrr: every candidate scored and sorted, 1/rank
of the first relevant one wherever it is) need neither the score block nor a sort:
    rank_i = 1 + #{ j : s_ij beats the best relevant document of query i }
first_relevant_rank takes the best relevant score and column per query (tt_rank_best_relevant)
and counts the columns that beat it (tt_rank_count: for bf16 and h in {128, 256, 512} the
streamed MFMA scan with a counting epilogue); mrr_from_ranks / recall_from_ranks turn the
ranks into the metrics for any k, and validate_full_rank is the sampling loop of
validate_margin.py:105-148.
"""
from __future__ import annotations

import random
from typing import Sequence

import torch

from . import _lib, ops
from ._lib import call, dtype_code, stream_ptr
from .data import encode_batch
from .losses import mine_hard_negatives


@torch.no_grad()
def encode_texts(model, texts: Sequence[str], vocab, kind: str, max_length: int = 30, batch: int = 4096,
                 device="cuda", tokenize=None) -> torch.Tensor:
    """[len(texts), h] fp32 tower outputs; kind is 'query' or 'doc'. tokenize(texts, vocab,
    max_length) -> int32 [n, max_length] row ids (default data.encode_batch)."""
    encode_batch_ = tokenize or encode_batch
    was = model.training
    model.eval()
    outs = []
    enc = model.encode_query if kind == "query" else model.encode_doc
    for i in range(0, len(texts), batch):
        ids = encode_batch_(texts[i:i + batch], vocab, max_length).to(device)
        outs.append(enc(ids))
    model.train(was)
    return torch.cat(outs, 0)


@torch.no_grad()
def topk_cosine(query_vecs: torch.Tensor, doc_vecs: torch.Tensor, k: int = 10, compute_dtype=torch.float32):
    """Top-k documents per query by cosine similarity: (indices int64 [Q,k], scores [Q,k]).
    compute_dtype=torch.int8: both sides are normalised (eps 1e-8), quantised row by row
    (ops.quantize_rows_i8) and searched with tt_search_topk_i8; the scores are the int8
    approximation of the cosines (no rescoring)."""
    if compute_dtype == torch.int8:
        _lib.require_gpu(query_vecs, doc_vecs)
        kmax, nd = _lib.topk_max(), doc_vecs.shape[0]
        if not 1 <= k <= min(kmax, nd):
            raise ValueError(f"k={k} needs 1 <= k <= min({kmax}, {nd} documents)")
        qn, _, _ = ops.l2norm_fwd(query_vecs.float().contiguous(), 1e-8, torch.float32)
        dn, _, _ = ops.l2norm_fwd(doc_vecs.float().contiguous(), 1e-8, torch.float32)
        idx, val = ops.search_topk_i8(*ops.quantize_rows_i8(qn), *ops.quantize_rows_i8(dn), k)
        return idx.long(), val
    idx, val = mine_hard_negatives(query_vecs, doc_vecs, label_offset=-1, k=k, compute_dtype=compute_dtype,
                                   return_values=True)
    return idx.long(), val


def mrr_at_k(top_idx: torch.Tensor, relevant: Sequence[set]) -> float:
    """Mean over queries of 1/rank of the first relevant document in top_idx (0 if none)."""
    total = 0.0
    rows = top_idx.cpu().tolist()
    for row, rel in zip(rows, relevant):
        for rank, j in enumerate(row, 1):
            if j in rel:
                total += 1.0 / rank
                break
    return total / max(len(rows), 1)


def recall_at_k(top_idx: torch.Tensor, relevant: Sequence[set], ks: Sequence[int] = (1, 3, 10)) -> dict:
    """{k: share of queries with a relevant document within the first k of top_idx}
    (compare_models.py:60-84, R@1 / R@3 / R@10); k beyond top_idx's width counts the whole row."""
    rows = top_idx.cpu().tolist()
    hits = {int(k): 0 for k in ks}
    for row, rel in zip(rows, relevant):
        first = next((rank for rank, j in enumerate(row, 1) if j in rel), None)
        if first is not None:
            for k in hits:
                hits[k] += first <= k
    return {k: n / max(len(rows), 1) for k, n in hits.items()}


# ------------------------------------------------------------------------- full ranks
def relevance_csr(relevant):
    """A sequence of iterables of document indices as CSR: (ptr int32 [Q + 1], idx int32),
    each row's indices sorted and de-duplicated."""
    ptr, idx = [0], []
    for rel in relevant:
        row = sorted({int(j) for j in rel})
        idx.extend(row)
        ptr.append(len(idx))
    if len(idx) >= 2 ** 31:
        raise _lib.TTError("relevance_csr: more than 2^31 - 1 entries")
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(idx, dtype=torch.int32)


def _as_csr(relevant, Q: int, N: int):
    if len(relevant) == 2 and isinstance(relevant[0], torch.Tensor) and isinstance(relevant[1], torch.Tensor):
        ptr, idx = relevant
    else:
        ptr, idx = relevance_csr(relevant)
    if ptr.numel() != Q + 1:
        raise _lib.TTError(f"first_relevant_rank: relevance has {ptr.numel() - 1} rows for {Q} queries")
    if idx.device.type == "cpu" and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise _lib.TTError(f"first_relevant_rank: relevant document index outside [0, {N})")
    return ptr, idx


@torch.no_grad()
def first_relevant_rank(query_vecs: torch.Tensor, doc_vecs: torch.Tensor, relevant, compute_dtype=torch.float32,
                        eps: float = 1e-8, doc_block: int | None = None) -> torch.Tensor:
    """int32 [Q]: the 1-based position of each query's first relevant document in the full
    descending cosine order over ALL documents (equal scores towards the lower document
    index, the order of topk_cosine and of the reference's stable sort); 0 for a query
    without relevant documents. relevant: a sequence of sets of document indices (as
    mrr_at_k takes) or the (ptr, idx) pair of relevance_csr. doc_block: count the documents
    in blocks of that many rows (the thresholds are taken over all of them first)."""
    _lib.require_gpu(query_vecs, doc_vecs)
    lib = _lib.load()
    Q, N = query_vecs.shape[0], doc_vecs.shape[0]
    dev = query_vecs.device
    ptr, idx = _as_csr(relevant, Q, N)
    ranks = torch.zeros(Q, dtype=torch.int32, device=dev)
    if Q == 0:
        return ranks
    ptr = ptr.to(device=dev, dtype=torch.int32).contiguous()
    idx = idx.to(device=dev, dtype=torch.int32).contiguous()
    qn, _, _ = ops.l2norm_fwd(query_vecs.float().contiguous(), eps, compute_dtype, want_f32=False)
    dn, _, _ = ops.l2norm_fwd(doc_vecs.float().contiguous(), eps, compute_dtype, want_f32=False)
    h = qn.shape[1]
    dc = dtype_code(compute_dtype)
    theta = torch.empty(Q, dtype=torch.float32, device=dev)
    tcol = torch.empty(Q, dtype=torch.int32, device=dev)
    count = torch.empty(Q, dtype=torch.int32, device=dev)
    st = stream_ptr(dev)
    call("tt_rank_best_relevant", dc, qn.data_ptr(), Q, dn.data_ptr(), N, h, ptr.data_ptr(), idx.data_ptr(),
         theta.data_ptr(), tcol.data_ptr(), None, st)
    step = N if not doc_block else max(1, int(doc_block))
    for b0 in range(0, max(N, 1), max(step, 1)):
        n = min(N, b0 + step) - b0
        ws = torch.empty(lib.tt_rank_count_ws_size(dc, Q, n, h), dtype=torch.uint8, device=dev)
        call("tt_rank_count", dc, qn.data_ptr(), Q, dn[b0:].data_ptr(), n, h, b0, theta.data_ptr(), tcol.data_ptr(),
             count.data_ptr(), 1 if b0 else 0, ws.data_ptr(), st)
    return torch.where(tcol >= 0, count + 1, ranks)


def mrr_from_ranks(ranks) -> float:
    """Mean of 1/rank over the queries; rank 0 (no relevant document) counts 0."""
    r = torch.as_tensor(ranks).double().cpu().reshape(-1)
    if r.numel() == 0:
        return 0.0
    return float(torch.where(r > 0, 1.0 / r.clamp_min(1.0), torch.zeros_like(r)).mean())


def recall_from_ranks(ranks, ks: Sequence[int] = (1, 3, 10)) -> dict:
    """{k: share of queries whose first relevant document ranks within the first k}; rank 0
    is a miss."""
    r = torch.as_tensor(ranks).long().cpu().reshape(-1)
    n = max(r.numel(), 1)
    return {int(k): int(((r > 0) & (r <= int(k))).sum()) / n for k in ks}


def _tokenizer_of(model):
    from .margin import TwoTowerModel, margin_ids
    if isinstance(model, TwoTowerModel):  # SimpleDataset.text_to_embedding's marker rewriting
        return lambda texts, vocab, max_length: torch.tensor([margin_ids(t, vocab, max_length) for t in texts],
                                                             dtype=torch.int32)
    return None


def validate_full_rank(model, vocab, queries: Sequence[str], docs: Sequence[str], relevant: Sequence[set],
                       num_queries: int = 20, seed=None, out_path: str | None = None, device="cuda") -> dict:
    """The validation loop of validate_margin.py:105-148 over full ranks: sample num_queries
    of the queries that have relevant documents (random.Random(seed); the reference samples
    unseeded), encode them and every document, take each query's full rank and its top 3,
    and return {"query_index", "rank", "reciprocal_rank", "top3", "top3_scores", "mrr"} (mrr
    the average reciprocal rank). relevant[i]: the set of indices into docs relevant to
    queries[i]. out_path: append the reference's per-query block (:139-146). The model needs
    its embedding table attached (set_embedding_table) for the token-id inputs."""
    valid = [i for i, rel in enumerate(relevant) if rel]
    if len(valid) > num_queries:
        valid = random.Random(seed).sample(valid, num_queries)
    tok = _tokenizer_of(model)
    dv = encode_texts(model, list(docs), vocab, "doc", device=device, tokenize=tok)
    qv = encode_texts(model, [queries[i] for i in valid], vocab, "query", device=device, tokenize=tok) if valid else \
        dv[:0]
    rel = [relevant[i] for i in valid]
    ranks = first_relevant_rank(qv, dv, rel).cpu().tolist() if valid else []
    k = min(3, len(docs))
    if valid and k:
        ti, tv = topk_cosine(qv, dv, k=k)
        ti, tv = ti.cpu().tolist(), tv.cpu().tolist()
    else:
        ti, tv = [[] for _ in valid], [[] for _ in valid]
    rr = [1.0 / r if r > 0 else 0.0 for r in ranks]
    if out_path is not None:
        with open(out_path, "a", encoding="utf-8") as f:
            for i, m, row, sc in zip(valid, rr, ti, tv):
                truth = docs[min(relevant[i])]
                f.write(f"\nQuery: {queries[i]}\n")
                f.write(f"Ground Truth Answer: {truth}\n")
                f.write(f"Ground Truth Passage: {truth}\n")
                f.write(f"MRR: {m:.4f}\n")
                for rank, (j, s) in enumerate(zip(row, sc), 1):
                    mark = "✓" if j in relevant[i] else " "
                    f.write(f"{rank}. [{mark}] ({s:.4f}) {docs[j][:100]}...\n")
    return {"query_index": valid, "rank": ranks, "reciprocal_rank": rr, "top3": ti, "top3_scores": tv,
            "mrr": sum(rr) / len(rr) if rr else 0.0}
