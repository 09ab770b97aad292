"""Sequence CTR model with DIN-style target attention over raw slots.

A raw (sequence) slot arrives as ``(B, sample_fixed_size, dim+1)`` with the
0/1 mask as the last channel; ``TargetAttentionPool`` reduces it to ``(B,
dim)`` with the candidate item's embedding (a sum slot of the same dim) as
the query — scaled dot-product scores, softmax over the valid cells, weighted
sum of the rows (ops/seqattn.py: one HIP kernel per direction on the GPU, the
torch reference on CPU).  ``ActivationUnitPool`` is DIN's own attention: a
small MLP over ``[q, k, q-k, q*k]`` scores each row and the scores weight a
plain sum, without a softmax (ops/actunit.py, MFMA kernels on the GPU).
``InterestGRUPool`` models the order of the sequence: a GRU over the rows,
or DIEN's attention-gated AUGRU, whose last state is the pooled vector
(ops/seqgru.py, a persistent MFMA kernel per direction on the GPU).
``SelfAttentionPool`` first lets the rows attend to each other (multi-head
self-attention, ops/seqsa.py, one MFMA kernel per direction; past 64 rows
ops/seqsal.py, which streams the keys) and then pools the result with the
target attention above.  Samples too long for the pooling kernel's LDS image
are pooled by ops/seqattnl.py, which streams the rows.  ``SeqEncoderLayer`` is the whole post-norm transformer block -- that self-attention followed by the
out-projection, add & LayerNorm and the feed-forward (ops/seqffn.py, one more
MFMA kernel per direction) -- under ``nn.TransformerEncoderLayer``'s parameter
names."""
import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from persia_amd.ops import native_available
from persia_amd.ops.actunit import act_unit_pool
from persia_amd.ops.seqattn import seq_attn_pool
from persia_amd.ops.seqattnl import prefers_long, seq_attn_pool_long
from persia_amd.ops.seqgru import seq_gru
from persia_amd.ops.seqffn import seq_ffn
from persia_amd.ops.seqsa import seq_self_attn
from persia_amd.ops.seqsal import seq_self_attn_long


def _self_attn(seq, *args, **kwargs):
    """``seq_self_attn`` up to its 64 rows, ``seq_self_attn_long`` past them."""
    fn = seq_self_attn if seq.shape[1] <= 64 else seq_self_attn_long
    return fn(seq, *args, **kwargs)


def _attn_pool(q, seq, scale=None):
    """``seq_attn_pool`` where its kernel takes the sample, on the GPU
    ``seq_attn_pool_long`` past that (``ops.seqattnl.prefers_long``)."""
    long = (q.is_cuda and seq.is_cuda and q.dim() == 2 and seq.dim() == 3
            and native_available() and prefers_long(seq.shape[1], q.shape[1]))
    return (seq_attn_pool_long if long else seq_attn_pool)(q, seq, scale)


class TargetAttentionPool(nn.Module):
    """forward(query [B, D], seq [B, L, D+1]) -> [B, D]; scale 1/sqrt(D)
    unless given."""

    def __init__(self, scale: Optional[float] = None):
        super().__init__()
        self.scale = scale

    def forward(self, query: torch.Tensor, seq: torch.Tensor) -> torch.Tensor:
        return _attn_pool(query, seq, self.scale)


class ActivationUnitPool(nn.Module):
    """DIN's local activation unit: forward(query [B, D], seq [B, L, D+1]) ->
    [B, D] = sum over the valid rows k_l of (w2 . sigmoid(W1 [q; k_l; q-k_l;
    q*k_l] + b1) + b2) * k_l.  The parameters are f32 masters."""

    def __init__(self, dim: int, hidden: int = 32):
        super().__init__()
        self.dim, self.hidden = dim, hidden
        bound1, bound2 = 1.0 / math.sqrt(4 * dim), 1.0 / math.sqrt(hidden)
        self.W1 = nn.Parameter(torch.empty(hidden, 4 * dim).uniform_(-bound1, bound1))
        self.b1 = nn.Parameter(torch.empty(hidden).uniform_(-bound1, bound1))
        self.w2 = nn.Parameter(torch.empty(hidden).uniform_(-bound2, bound2))
        self.b2 = nn.Parameter(torch.empty(()).uniform_(-bound2, bound2))

    def forward(self, query: torch.Tensor, seq: torch.Tensor) -> torch.Tensor:
        return act_unit_pool(query, seq, self.W1, self.b1, self.w2, self.b2)


class InterestGRUPool(nn.Module):
    """forward(query [B, D], seq [B, L, D+1]) -> [B, hidden]: the state of a
    GRU over the rows after the last valid one.  Parameters are f32 masters in
    ``torch.nn.GRU``'s layout and init (``weight_ih_l0`` ...), so a trained
    ``nn.GRU``'s state dict loads unchanged.  With ``attention=True`` the
    update gate of every row is scaled by its attention weight -- the softmax
    over the valid rows of <q, k_l>/sqrt(D), zero for a sample without a valid
    row -- which is DIEN's AUGRU; the query is ignored otherwise."""

    def __init__(self, dim: int, hidden: Optional[int] = None,
                 attention: bool = False):
        super().__init__()
        self.dim, self.hidden = dim, dim if hidden is None else hidden
        self.attention = attention
        bound = 1.0 / math.sqrt(self.hidden)
        for name, shape in (("weight_ih_l0", (3 * self.hidden, dim)),
                            ("weight_hh_l0", (3 * self.hidden, self.hidden)),
                            ("bias_ih_l0", (3 * self.hidden,)),
                            ("bias_hh_l0", (3 * self.hidden,))):
            setattr(self, name,
                    nn.Parameter(torch.empty(*shape).uniform_(-bound, bound)))

    def attention_weights(self, query: torch.Tensor, seq: torch.Tensor):
        """-> f32 [B, L]: softmax of <q, k_l>/sqrt(D) over the valid rows."""
        valid = seq[..., self.dim] != 0
        k = torch.where(valid.unsqueeze(-1), seq[..., :self.dim].float(),
                        torch.zeros((), device=seq.device))
        s = (k * query.float().unsqueeze(1)).sum(-1) * self.dim ** -0.5
        s = s.masked_fill(~valid, float("-inf"))
        m = s.max(dim=1, keepdim=True).values
        e = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
        den = e.sum(dim=1, keepdim=True)
        return e / torch.where(den > 0, den, torch.ones_like(den))

    def forward(self, query: torch.Tensor, seq: torch.Tensor) -> torch.Tensor:
        att = self.attention_weights(query, seq) if self.attention else None
        return seq_gru(seq, self.weight_ih_l0, self.weight_hh_l0,
                       self.bias_ih_l0, self.bias_hh_l0, att)[1]


class SelfAttentionLayer(nn.Module):
    """forward(seq [B, L, D+1], Wqkv, bqkv) -> [B, L, D+1]: ``seq_self_attn``
    with a residual; holds no parameters of its own."""

    def __init__(self, heads: int, causal: bool = False):
        super().__init__()
        self.heads, self.causal = heads, causal

    def forward(self, seq, Wqkv, bqkv) -> torch.Tensor:
        return _self_attn(seq, Wqkv, bqkv, self.heads, self.causal,
                          residual=True)


class _InProj(nn.Module):
    """The parameters of ``nn.MultiheadAttention``, under its names."""

    def __init__(self, dim: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dim))
        nn.init.xavier_uniform_(self.in_proj_weight)
        self.out_proj = nn.Linear(dim, dim)
        nn.init.zeros_(self.out_proj.bias)


class SeqEncoderLayer(nn.Module):
    """forward(seq [B, L, D+1]) -> [B, L, D+1]: a post-norm transformer
    encoder layer (ReLU, no dropout) among the valid rows of a raw slot --
    BST's layer, SASRec's with ``causal`` -- as ``seq_self_attn`` followed by
    ``seq_ffn``.  The parameters are f32 masters with the names, layouts and
    init of ``nn.TransformerEncoderLayer(dim, heads, ffn, dropout=0.0)``, so
    ``load_state_dict(nn_layer.state_dict())`` works."""

    def __init__(self, dim: int, heads: int, ffn: int, causal: bool = False,
                 eps: float = 1e-5):
        super().__init__()
        assert dim % heads == 0, f"{heads} heads do not divide dim {dim}"
        self.dim, self.heads, self.ffn, self.causal = dim, heads, ffn, causal
        self.self_attn = _InProj(dim)
        self.linear1, self.linear2 = nn.Linear(dim, ffn), nn.Linear(ffn, dim)
        self.norm1, self.norm2 = nn.LayerNorm(dim, eps=eps), nn.LayerNorm(dim, eps=eps)

    def forward(self, seq: torch.Tensor) -> torch.Tensor:
        sa, n1, n2 = self.self_attn, self.norm1, self.norm2
        a = _self_attn(seq, sa.in_proj_weight, sa.in_proj_bias, self.heads,
                       self.causal, residual=False)
        return seq_ffn(seq, a, sa.out_proj.weight, sa.out_proj.bias, n1.weight,
                       n1.bias, self.linear1.weight, self.linear1.bias,
                       self.linear2.weight, self.linear2.bias, n2.weight,
                       n2.bias, n1.eps)


class SelfAttentionPool(nn.Module):
    """forward(query [B, D], seq [B, L, D+1]) -> [B, D]: multi-head
    self-attention among the valid rows with a residual (``causal``: a row
    sees the rows not after it, as in SASRec; otherwise all of them, as in
    the Behavior Sequence Transformer), then target attention of the
    candidate over the result.  ``in_proj_weight`` / ``in_proj_bias`` are f32
    masters in ``torch.nn.MultiheadAttention``'s layout and init, so a trained
    module's tensors load unchanged.  With ``ffn`` given the rows run
    through a whole ``SeqEncoderLayer`` (``self.encoder``) with that hidden
    width instead, and its output is pooled."""

    def __init__(self, dim: int, heads: int = 2, causal: bool = False,
                 ffn: Optional[int] = None):
        super().__init__()
        assert dim % heads == 0, f"{heads} heads do not divide dim {dim}"
        self.dim, self.heads, self.causal = dim, heads, causal
        if ffn is not None:
            self.encoder = SeqEncoderLayer(dim, heads, ffn, causal)
            return
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dim))
        nn.init.xavier_uniform_(self.in_proj_weight)
        self.layer = SelfAttentionLayer(heads, causal)

    def forward(self, query: torch.Tensor, seq: torch.Tensor) -> torch.Tensor:
        if hasattr(self, "encoder"):
            return _attn_pool(query, self.encoder(seq))
        return _attn_pool(
            query, self.layer(seq, self.in_proj_weight, self.in_proj_bias))


class SeqCTR(nn.Module):
    """``dims[i]`` is the dim of embedding tensor i (in ``embedding_tensors``
    order); ``seq_query`` maps the index of each sequence tensor to the index
    of the sum slot that is its query.  Every sequence is pooled to ``(B,
    dim)``; the pooled vectors, all sum slots (queries included) and the dense
    features are concatenated and run through an MLP to one logit.

    ``fused=True`` runs the MLP on the MFMA kernels (ops/dense.py FusedMLP,
    hidden widths % 32 == 0) in bf16, with the input zero-padded to a
    multiple of 32 as in DCNv2.

    ``attention="dot"`` pools with ``TargetAttentionPool``; ``"mlp"`` gives
    every sequence an ``ActivationUnitPool`` of its own with ``att_hidden``
    hidden units (``self.act_pools[str(index)]``); ``"gru"`` and ``"augru"``
    give it an ``InterestGRUPool`` (``self.gru_pools[str(index)]``) whose
    hidden size is the slot's dim, so the MLP's input width stays what it
    is; ``"self"`` gives it a ``SelfAttentionPool`` with ``heads`` heads
    (``self.sa_pools[str(index)]``); ``"bst"`` gives that pool a whole
    encoder layer with ``ffn`` hidden units (default ``4 * dim``)."""

    def __init__(
        self,
        dims: Sequence[int],
        seq_query: Dict[int, int],
        num_dense: int = 13,
        hidden: Sequence[int] = (256, 128),
        fused: bool = False,
        attention: str = "dot",
        att_hidden: int = 32,
        heads: int = 2,
        ffn: Optional[int] = None,
    ):
        super().__init__()
        for s, qi in seq_query.items():
            assert qi not in seq_query, f"query {qi} of sequence {s} is a sequence"
            assert dims[s] == dims[qi], \
                f"sequence {s} (dim {dims[s]}) and its query {qi} (dim {dims[qi]})"
        self.seq_query = {int(s): int(qi) for s, qi in seq_query.items()}
        self.num_dense = num_dense
        assert attention in ("dot", "mlp", "gru", "augru", "self", "bst"), \
            attention
        self.attention = attention
        if attention == "dot":
            self.pool = TargetAttentionPool()
        elif attention in ("gru", "augru"):
            self.gru_pools = nn.ModuleDict({
                str(s): InterestGRUPool(dims[s], attention=attention == "augru")
                for s in sorted(self.seq_query)})
        elif attention in ("self", "bst"):
            self.sa_pools = nn.ModuleDict({
                str(s): SelfAttentionPool(
                    dims[s], heads,
                    ffn=None if attention == "self" else ffn or 4 * dims[s])
                for s in sorted(self.seq_query)})
        else:
            self.act_pools = nn.ModuleDict({
                str(s): ActivationUnitPool(dims[s], att_hidden)
                for s in sorted(self.seq_query)})
        in_dim = num_dense + sum(dims)
        self.fused = fused
        self.pad = (-in_dim) % 32 if fused else 0
        in_dim += self.pad
        sizes = [in_dim] + list(hidden) + [1]
        if fused:
            from persia_amd.ops.dense import FusedMLP

            self.mlp = FusedMLP(sizes)
        else:
            layers: List[nn.Module] = []
            for i in range(len(sizes) - 1):
                layers.append(nn.Linear(sizes[i], sizes[i + 1]))
                if i < len(sizes) - 2:
                    layers.append(nn.ReLU())
            self.mlp = nn.Sequential(*layers)

    def forward(self, non_id_tensors, embedding_tensors) -> torch.Tensor:
        dt = torch.bfloat16 if self.fused else torch.float32
        feats = []
        if self.num_dense:
            dense = (non_id_tensors if torch.is_tensor(non_id_tensors)
                     else non_id_tensors[0])
            feats.append(dense.to(dt))
        for i, e in enumerate(embedding_tensors):
            qi = self.seq_query.get(i)
            if qi is not None:
                pool = (self.pool if self.attention == "dot"
                        else self.act_pools[str(i)] if self.attention == "mlp"
                        else self.sa_pools[str(i)] if self.attention in ("self", "bst")
                        else self.gru_pools[str(i)])
                e = pool(embedding_tensors[qi], e)
            feats.append(e.to(dt))
        x = torch.cat(feats, dim=1)
        if self.pad:
            x = torch.nn.functional.pad(x, (0, self.pad))
        return self.mlp(x).squeeze(1).float()
