"""A trainable (or frozen) embedding table for the token-id inputs of the towers.

The reference's first prototype has the switch (train_two_tower.py:29,
pretrained_embeddings=..., freeze_embeddings=True); here the table stays outside the model:

    table = tta.EmbeddingTable(vocab, trainable=True).to("cuda")
    model.set_embedding_table(table)
    opt_e = tta.SparseAdam(table.parameters(), lr=1e-3)

`weight` is the fp32 master [V, E]. The kernels gather from a copy of it in the model's
compute dtype, zero-padded to the GEMM's column multiple ([V, Ep], ops.pad_cols). The copy
follows weight._version like the packed-weight cache of the towers: optim.SparseAdam rewrites
the rows it touched in place and records the version it produced; any other writer
(torch.optim.SparseAdam, load_state_dict, copy_) makes the next use rebuild it whole. Writes
through `.data` leave the version alone; a fixed sample of weight is compared as well, which
catches a replaced table (EmbeddingTable._sample).

After a backward, weight.grad is a coalesced torch.sparse_coo_tensor [V, E] whose indices
are the distinct ids of the batch: nn.Embedding(sparse=True)'s contract.

Under data parallelism the table opts in with table.set_process_group(group): the indices are
then the distinct ids of the global batch and the values the sums over all ranks, the same bits
on every rank (towers.py, dist.union_ids).

The module is never registered as a submodule of a model (the reference's state_dict keys
stay); it has its own state_dict.
"""
from __future__ import annotations

import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib, dist, ops

_tables: "weakref.WeakSet[EmbeddingTable]" = weakref.WeakSet()
_NSAMPLE = 4096


class EmbeddingTable(nn.Module):
    def __init__(self, weight_or_vocab, trainable: bool = True):
        super().__init__()
        w = weight_or_vocab
        if hasattr(w, "vectors") and not isinstance(w, torch.Tensor):  # data.Vocab / gensim KeyedVectors
            w = w.vectors
        if isinstance(w, np.ndarray):
            w = torch.from_numpy(np.array(w, dtype=np.float32))
        if not isinstance(w, torch.Tensor):
            raise TypeError("EmbeddingTable expects a [V, E] tensor, array or Vocab")
        if w.dim() != 2 or w.shape[0] < 1 or w.shape[1] < 1 or not w.is_floating_point():
            raise ValueError(f"EmbeddingTable weight must be a float [V, E] matrix, got {w.dtype} {tuple(w.shape)}")
        if w.shape[0] >= 2 ** 31:
            raise ValueError("EmbeddingTable rows are addressed by int32 token ids")
        self.weight = nn.Parameter(w.detach().to(torch.float32).clone().contiguous(), requires_grad=bool(trainable))
        self._copy = None  # (key, [V, Ep] compute-dtype copy, sample of weight)
        self.dp_group = None  # (group,) once set_process_group has opted in to data parallelism
        _tables.add(self)

    @property
    def trainable(self) -> bool:
        return self.weight.requires_grad

    @property
    def num_embeddings(self) -> int:
        return self.weight.shape[0]

    @property
    def embedding_dim(self) -> int:
        return self.weight.shape[1]

    def set_process_group(self, group=None):
        """Train this table under data parallelism over `group` (None: the default group). Each
        backward then leaves the same coalesced sparse gradient on every rank: the rows of the
        ids any rank saw, summed across ranks (towers.py, dist.union_ids), so the same
        SparseAdam step everywhere keeps the tables and their moments bit-identical. Rank 0's
        weight is broadcast once, here. Without an active group the table trains as on one rank."""
        self.dp_group = (group,)
        if dist.active(group):
            src = 0 if group is None else torch.distributed.get_global_rank(group, 0)
            with torch.no_grad():
                torch.distributed.broadcast(self.weight, src, group=group)
            torch.autograd.graph.increment_version(self.weight)  # written in place: the compute copy rebuilds
        return self

    def _key(self, dt, ep):
        w = self.weight
        return (dt, ep, w.device, w.data_ptr(), w._version)

    def _sample(self) -> torch.Tensor:
        """Up to _NSAMPLE elements of weight at a fixed odd stride. Writes through `.data`
        bypass version tracking (weight.data.copy_(new_vectors) is how pretrained vectors are
        usually swapped in); a changed sample catches every such write that replaces the
        table, though not one that touches only elements between the sampled ones."""
        flat = self.weight.detach().view(-1)
        stride = max(1, flat.numel() // _NSAMPLE) | 1
        return flat[::stride][:_NSAMPLE].clone()

    def device_copy(self, device, dt: torch.dtype) -> torch.Tensor:
        """The padded compute-dtype copy the gather reads, rebuilt when weight has changed
        since the copy was made (or last kept in step by optim.SparseAdam)."""
        w = self.weight
        d = torch.device(device)
        if w.device.type != d.type or (d.index is not None and w.device.index != d.index):
            raise _lib.TTError(f"EmbeddingTable is on '{w.device}' but the inputs are on '{d}': move the table "
                               "to the GPU (table.to('cuda')); it is not a submodule of the model")
        ep = ops.pad_cols(w.shape[1], dt)
        key = self._key(dt, ep)
        if self._copy is not None and self._copy[0] == key and torch.equal(self._copy[2], self._sample()):
            return self._copy[1]
        with torch.no_grad():
            t = torch.zeros(w.shape[0], ep, dtype=dt, device=w.device)
            t[:, : w.shape[1]] = w.detach().to(dt)
        t.real_cols = w.shape[1]  # for algorithmic-byte accounting (timing.py)
        self._copy = (key, t, self._sample())
        return t

    def current_copy(self):
        """The compute copy if it was made from weight's current version, else None."""
        if self._copy is None:
            return None
        key, t, _ = self._copy
        return t if key == self._key(key[0], key[1]) else None

    def copy_updated(self):
        """The rows of the copy that weight's last writer changed have been rewritten (by
        tt_sparse_adam_rows): the copy now stands for weight's current version."""
        if self._copy is not None:
            key, t, _ = self._copy
            self._copy = (self._key(key[0], key[1]), t, self._sample())

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        raise _lib.TTError("EmbeddingTable is read by the towers' gather kernel: attach it with "
                           "model.set_embedding_table(table) and pass [B, T] token ids to the model")


def keep_coalesced(param):
    """Post-accumulate-grad hook of a weight that takes the towers' sparse gradient (set by
    TowersFn.forward). autograd stores a sparse gradient as a shallow copy (same indices and
    values) that has lost its coalesced flag. When .grad holds exactly the indices the towers'
    backward made
    (param._tt_grad_ids: distinct and ascending by construction), say so again; a gradient
    accumulated over several backward passes has other indices and stays as autograd left it."""
    g, ids = param.grad, getattr(param, "_tt_grad_ids", None)
    if (g is not None and ids is not None and g.is_sparse and not g.is_coalesced() and g._nnz() == ids.numel() > 0
            and g._indices().data_ptr() == ids.data_ptr()):
        g._coalesced_(True)


def table_of(param) -> "EmbeddingTable | None":
    """The EmbeddingTable whose weight is this parameter, if any."""
    for t in list(_tables):
        if t.weight is param:
            return t
    return None


def trainable_table(model, device_table) -> "EmbeddingTable | None":
    """The model's EmbeddingTable if this call gathers from it (device_table is its copy)
    and its weight takes a gradient; None for a frozen table or float inputs."""
    src = getattr(model, "_table_src", None)
    if device_table is None or not isinstance(src, EmbeddingTable):
        return None
    return src if src.weight.requires_grad and torch.is_grad_enabled() else None


def check_table(table, embedding_dim: int):
    """Validation shared by the models' set_embedding_table."""
    if isinstance(table, EmbeddingTable):
        if table.embedding_dim != embedding_dim:
            raise ValueError(f"table must be [V, {embedding_dim}]")
    elif table is not None and (table.dim() != 2 or table.shape[1] != embedding_dim):
        raise ValueError(f"table must be [V, {embedding_dim}]")
