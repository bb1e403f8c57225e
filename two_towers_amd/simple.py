"""The Simple two-tower recipe (simple_two_tower.py) on the HIP path.

  SimpleTwoTower(embedding_dim, hidden_dim)   simple_two_tower.py:14-66
        two nn.GRU(E, hidden_dim, 2 layers, bidirectional, dropout 0.1) encoders and one
        projection per tower, Sequential(Linear(2H,H), LayerNorm(H), ReLU, Dropout(0.1),
        Linear(H,H/2)); same submodule names, hence the same 44 state_dict keys and the
        same default initialisation for a given torch seed. forward / encode_query /
        encode_doc return L2-normalised vectors [B, H/2].
  InfoNCELoss(temperature=0.1)                simple_two_tower.py:68-78, the symmetric
        loss: losses.SymmetricInfoNCELoss.
  SimpleDataset                               simple_two_tower.py:80-118, the featurisation
        rule of EnhancedDataset (data.EnhancedDataset).

The inner loop of simple_two_tower.py:229-240 runs as

    optimizer = AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)   # optim.AdamW
    loss = InfoNCELoss(0.1)(*model(q, d)); loss.backward()
    clip_grad_norm_(model.parameters(), 1.0); optimizer.step()          # optim.clip_grad_norm_

GPU layout: the GRU towers are the fused TowersFn with cfg.head "none" (margin.py); each
tower then takes its own tt_proj_head1 call (Linear(2H,H) + LayerNorm + ReLU + Dropout),
Linear(H,H/2) as tt_gemm products (forward with the bias epilogue; backward dx, dW and the
column-sum db) and tt_l2norm.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, ops
from .data import EnhancedDataset as SimpleDataset
from .losses import SymmetricInfoNCELoss
from .margin import TwoTowerModel as _Margin
from .margin import _SharedHeadFn, normalize
from .optim import AdamW, clip_grad_norm_


class _LinearFn(torch.autograd.Function):
    """x [rows, K] fp32, w [N, K], b [N] -> x w^T + b on tt_gemm (fp32)."""

    @staticmethod
    def forward(ctx, x, w, b):
        _lib.require_gpu(x, w, b)
        x = x.float().contiguous()
        wd = w.detach().float().contiguous()
        bd = b.detach().float().contiguous()
        rows, K = x.shape
        N = wd.shape[0]
        if tuple(wd.shape) != (N, K) or tuple(bd.shape) != (N,):
            raise ValueError(f"linear expects weight [N, {K}] and bias [N], got {tuple(wd.shape)}, {tuple(bd.shape)}")
        out = torch.empty(rows, N, dtype=torch.float32, device=x.device)
        f32 = torch.float32
        ops.gemm([x], [wd], [out], m=rows, n=N, k=K, lda=K, ldb=K, ldc=N, a_kouter=False, b_kouter=False, dtype=f32,
                 out_dtype=f32, bias=[bd])
        ctx.save = (x, wd)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, w = ctx.save
        rows, K = x.shape
        N = w.shape[0]
        g = gout.float().contiguous()
        f32 = torch.float32
        dx = torch.empty(rows, K, dtype=f32, device=x.device)
        dw = torch.empty(N, K, dtype=f32, device=x.device)
        db = torch.empty(N, dtype=f32, device=x.device)
        # dx = g w (w read K-outer: [k = N][n = K]); dw = g^T x (both K-outer over the rows)
        ops.gemm([g], [w], [dx], m=rows, n=K, k=N, lda=N, ldb=K, ldc=K, a_kouter=False, b_kouter=True, dtype=f32,
                 out_dtype=f32)
        ops.gemm([g], [x], [dw], m=N, n=K, k=rows, lda=N, ldb=K, ldc=K, a_kouter=True, b_kouter=True, dtype=f32,
                 out_dtype=f32)
        ops.colsum(g, rows, N, N, db)
        ctx.save = None
        return dx, dw, db


def _proj(hidden_dim: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(hidden_dim * 2, hidden_dim), nn.LayerNorm(hidden_dim), nn.ReLU(), nn.Dropout(0.1),
                         nn.Linear(hidden_dim, hidden_dim // 2))


class SimpleTwoTower(nn.Module):
    def __init__(self, embedding_dim: int, hidden_dim: int):
        super().__init__()
        self.query_encoder = nn.GRU(input_size=embedding_dim, hidden_size=hidden_dim, num_layers=2,
                                    batch_first=True, bidirectional=True, dropout=0.1)
        self.doc_encoder = nn.GRU(input_size=embedding_dim, hidden_size=hidden_dim, num_layers=2,
                                  batch_first=True, bidirectional=True, dropout=0.1)
        self.query_proj = _proj(hidden_dim)
        self.doc_proj = _proj(hidden_dim)
        self.embedding_dim = embedding_dim
        self.hidden_dim = hidden_dim
        self.compute_dtype = torch.float32
        self._table = None
        self._table_src = None
        self.process_group = None
        self.overlap_grad_allreduce = False

    # options and the fused GRU towers: exactly margin.TwoTowerModel's
    set_process_group = _Margin.set_process_group
    set_compute_dtype = _Margin.set_compute_dtype
    set_embedding_table = _Margin.set_embedding_table
    _device_table = _Margin._device_table
    _towers = _Margin._towers

    def _head(self, proj: nn.Sequential, hidden: torch.Tensor) -> torch.Tensor:
        drop_p = float(proj[3].p) if self.training else 0.0
        u = _SharedHeadFn.apply(hidden, proj[0].weight, proj[0].bias, proj[1].weight, proj[1].bias, drop_p)
        return normalize(_LinearFn.apply(u, proj[4].weight, proj[4].bias))

    def encode_query(self, query_emb):
        return self._head(self.query_proj, self._towers(["query"], [query_emb])[0])

    def encode_doc(self, doc_emb):
        return self._head(self.doc_proj, self._towers(["doc"], [doc_emb])[0])

    def forward(self, query_emb, doc_emb):
        hq, hd = self._towers(["query", "doc"], [query_emb, doc_emb])
        return self._head(self.query_proj, hq), self._head(self.doc_proj, hd)


class InfoNCELoss(SymmetricInfoNCELoss):
    """simple_two_tower.py:68-78 (temperature 0.1, inputs already normalised)."""

    def __init__(self, temperature=0.1, compute_dtype=None, process_group=None):
        super().__init__(temperature=temperature, normalize=False, compute_dtype=compute_dtype,
                         process_group=process_group)


__all__ = ["SimpleTwoTower", "InfoNCELoss", "SimpleDataset", "AdamW", "clip_grad_norm_"]
