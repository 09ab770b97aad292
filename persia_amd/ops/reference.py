"""Pure-torch fp32 reference implementations of every sparse op.

These define the numerics contract the HIP kernels are tested against
(tests/test_gpu_kernels.py compares each HIP kernel with these on the same
inputs).  They also power the CPU execution path (job on a machine without a
GPU — reference parity: the adult-income CPU run).

Math sources (reference implementation):
* segment sum + sqrt scaling  — embedding_worker_service/mod.rs:486-629
* gradient scatter + scaling  — embedding_worker_service/mod.rs:703-872
* sparse optimizers           — rust/persia-simd/src/lib.rs (exact formulas)
"""
from typing import Optional, Tuple

import torch


# ---------------------------------------------------------------- forward ops


def segment_sum_rows(
    rows: torch.Tensor,  # [U, dim] f32 — unique rows
    inverse: torch.Tensor,  # [nnz] i64 — position -> unique row index
    seg_offsets: torch.Tensor,  # [n_seg + 1] i64 — CSR offsets of positions per segment
    sqrt_scaling: bool = False,
    out_dtype: torch.dtype = torch.float16,
) -> torch.Tensor:
    """out[s] = sum_{k in segment s} rows[inverse[k]]; optionally scaled by
    1/sqrt(max(len(segment), 1))."""
    n_seg = seg_offsets.numel() - 1
    dim = rows.shape[1]
    lens = (seg_offsets[1:] - seg_offsets[:-1]).to(rows.device)
    seg_ids = torch.repeat_interleave(
        torch.arange(n_seg, device=rows.device, dtype=torch.int64), lens
    )
    out = torch.zeros(n_seg, dim, dtype=torch.float32, device=rows.device)
    out.index_add_(0, seg_ids, rows.float()[inverse])
    if sqrt_scaling:
        scale = lens.clamp(min=1).float().rsqrt().unsqueeze(1)
        out = out * scale
    return out.to(out_dtype)


def raw_embedding_tensors(
    rows: torch.Tensor,  # [U_slot, dim] f32 — this slot's distinct rows (order = first occurrence in sorted-unique order)
    inverse: torch.Tensor,  # [nnz_slot] i64 — position -> distinct row index (0-based)
    seg_offsets: torch.Tensor,  # [B+1] i64
    sample_fixed_size: int,
    scale: float = 1.0,
    out_dtype: torch.dtype = torch.float16,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Build the reference raw-slot tensor contract
    (embedding_worker_service/mod.rs:593-629 + persia-core forward.rs:333-394):

    returns (distinct_with_pad [U+1, dim] out_dtype — row 0 zeros,
             index [B*sfs] i64 — 0 = padding, else distinct_idx+1,
             non_empty_index [k] i64 — positions in index that are non-zero,
             sample_id_num [B] i64).

    Note: when one sample holds more than ``sample_fixed_size`` ids, only the
    first ``sample_fixed_size`` are indexed (reference truncation).  A
    distinct id appearing twice in one sample occupies both columns.
    """
    device = rows.device
    B = seg_offsets.numel() - 1
    U = rows.shape[0]
    dim = rows.shape[1]
    distinct = torch.zeros(U + 1, dim, dtype=torch.float32, device=device)
    distinct[1:] = rows.float() * scale
    lens = seg_offsets[1:] - seg_offsets[:-1]
    index = torch.zeros(B * sample_fixed_size, dtype=torch.int64, device=device)
    # column index of each position within its sample
    pos = torch.arange(inverse.numel(), device=device, dtype=torch.int64)
    col = pos - seg_offsets[:-1].repeat_interleave(lens)
    sample = torch.arange(B, device=device, dtype=torch.int64).repeat_interleave(lens)
    keep = col < sample_fixed_size
    index[sample[keep] * sample_fixed_size + col[keep]] = inverse[keep] + 1
    non_empty_index = torch.nonzero(index, as_tuple=False).view(-1)
    sample_id_num = lens.clamp(max=sample_fixed_size)
    return distinct.to(out_dtype), index, non_empty_index, sample_id_num


# --------------------------------------------------------------- backward ops


def segment_grad_scatter(
    grads: torch.Tensor,  # [n_seg, dim] f16/f32 — per-(slot,sample) grads
    inverse: torch.Tensor,  # [nnz] i64 — position -> unique row index
    seg_offsets: torch.Tensor,  # [n_seg+1] i64
    n_unique: int,
    scale_factor: float = 1.0,
    sqrt_scaling: bool = False,
) -> torch.Tensor:
    """grad_out[u] = sum_{k: inverse[k]==u} grads[segment(k)] * scale
    where scale = (1/scale_factor) * (sqrt_scaling ? 1/sqrt(len(segment(k))) : 1).

    Mirror of the reference's per-sign AVX2 grad accumulation
    (mod.rs:782-814) with loss-scale recip (mod.rs:751-755) and sqrt scaling
    (mod.rs:757-777)."""
    n_seg = seg_offsets.numel() - 1
    dim = grads.shape[1]
    lens = (seg_offsets[1:] - seg_offsets[:-1]).to(grads.device)
    seg_ids = torch.repeat_interleave(
        torch.arange(n_seg, device=grads.device, dtype=torch.int64), lens
    )
    g = grads.float()
    if scale_factor != 1.0:
        g = g / scale_factor
    if sqrt_scaling:
        g = g * lens.clamp(min=1).float().rsqrt().unsqueeze(1)
    out = torch.zeros(n_unique, dim, dtype=torch.float32, device=grads.device)
    out.index_add_(0, inverse, g[seg_ids])
    return out


# ------------------------------------------------------- sparse optimizer math
# Row layout (reference emb_entry.rs:17-23): inner = [emb(dim) | opt_state].


def sgd_update(
    emb: torch.Tensor, grad: torch.Tensor, lr: float, wd: float, weight_bound: float
) -> None:
    """w -= lr*(g + wd*w); clamp ±weight_bound (persia-simd lib.rs:124-144, 231)."""
    emb -= lr * (grad + wd * emb)
    if weight_bound > 0:
        emb.clamp_(-weight_bound, weight_bound)


def adagrad_update(
    emb: torch.Tensor,  # [n, dim] f32
    accum: torch.Tensor,  # [n, dim] f32 (or [n, 1] vectorwise-shared)
    grad: torch.Tensor,  # [n, dim] f32
    lr: float,
    g_square_momentum: float,
    eps: float,
    weight_bound: float,
    vectorwise_shared: bool = False,
) -> None:
    """w -= lr * g * rsqrt(acc_old + eps);
    acc = acc_old * momentum + g²  (per-dim) or mean(g²) (shared)
    (persia-simd lib.rs:21-121 — accumulator is read BEFORE its update)."""
    if vectorwise_shared:
        emb -= lr * grad * torch.rsqrt(accum + eps)
        gsq = (grad * grad).mean(dim=1, keepdim=True)
        accum.mul_(g_square_momentum).add_(gsq)
    else:
        emb -= lr * grad * torch.rsqrt(accum + eps)
        accum.mul_(g_square_momentum).add_(grad * grad)
    if weight_bound > 0:
        emb.clamp_(-weight_bound, weight_bound)


def adam_update(
    emb: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    grad: torch.Tensor,
    beta1_power: float,
    beta2_power: float,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_bound: float,
) -> None:
    """Bias-corrected Adam (persia-simd lib.rs:147-228); β-powers are
    maintained per feature group per update batch (persia-common optim.rs:147-216)."""
    m.mul_(beta1).add_(grad, alpha=1.0 - beta1)
    v.mul_(beta2).add_(grad * grad, alpha=1.0 - beta2)
    m_hat = m / (1.0 - beta1_power)
    v_hat = v / (1.0 - beta2_power)
    emb -= lr * m_hat / (eps + v_hat.sqrt())
    if weight_bound > 0:
        emb.clamp_(-weight_bound, weight_bound)


def ftrl_update(
    emb: torch.Tensor,  # [n, dim] f32
    z: torch.Tensor,  # [n, dim] f32
    n: torch.Tensor,  # [n, dim] f32
    grad: torch.Tensor,  # [n, dim] f32
    lr: float,
    beta: float,
    l1: float,
    l2: float,
    weight_bound: float,
) -> None:
    """Per-coordinate FTRL-Proximal (McMahan et al. 2013, Algorithm 1; not in
    the reference): n += g²; z += g - sigma*w with sigma = (sqrt(n_new) -
    sqrt(n_old))/lr; w = (clip(z, ±l1) - z) / ((beta + sqrt(n_new))/lr + l2),
    which is exactly 0 where |z| <= l1.  The old weight enters only through
    sigma*w (csrc/optim.h pa_ftrl)."""
    s0 = n.sqrt()
    n.add_(grad * grad)
    s1 = n.sqrt()
    sigma = (s1 - s0) / lr
    z.add_(grad - sigma * emb)
    q = (beta + s1) / lr + l2
    emb.copy_((z.clamp(-l1, l1) - z) / q)
    if weight_bound > 0:
        emb.clamp_(-weight_bound, weight_bound)


# ------------------------------------------------- target-attention pooling


def seq_attn_pool_reference(
    q: torch.Tensor,  # [B, D]
    seq: torch.Tensor,  # [B, L, D+1] — channel D is the 0/1 mask
    scale: Optional[float] = None,
) -> torch.Tensor:
    """DIN-style target attention over a raw slot's tensor, plain torch (not
    in the reference; csrc/seqattn.hip is the HIP twin):

        s_l = scale * <q, k_l>,  p = softmax of s over the valid l,
        out = sum_{valid l} p_l * k_l                     -> [B, D], q's dtype

    with k_l = seq[:, l, :D] and valid_l = (seq[:, l, D] != 0); scale defaults
    to 1/sqrt(D).  The mask selects and never multiplies: an invalid row is
    replaced by zeros before any arithmetic, so an Inf or NaN there reaches
    neither the output nor a gradient.  A sample without a valid cell gives
    zeros.  Computes in f32 (f64 for f64 inputs); differentiable in q and seq
    (the mask channel's gradient is zero)."""
    D = q.shape[-1]
    if scale is None:
        scale = float(D) ** -0.5
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    valid = seq[..., D] != 0
    k = seq[..., :D].to(ct)
    k = torch.where(valid.unsqueeze(-1), k, torch.zeros((), dtype=ct, device=k.device))
    s = scale * (k * q.to(ct).unsqueeze(1)).sum(-1)
    s = s.masked_fill(~valid, float("-inf"))
    m = s.max(dim=1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)  # 0 at an invalid cell
    den = e.sum(dim=1, keepdim=True)
    p = e / torch.where(den > 0, den, torch.ones_like(den))
    return (p.unsqueeze(-1) * k).sum(dim=1).to(q.dtype)


# ------------------------------------------- activation-unit (MLP) pooling


def _round_f16_st(x: torch.Tensor) -> torch.Tensor:
    """x with the value of its f16 rounding (through f32, as the kernel
    rounds) and the gradient of the identity."""
    return x + (x.float().half().to(x.dtype) - x).detach()


def act_unit_prepared_reference(
    q: torch.Tensor,  # [B, D]
    seq: torch.Tensor,  # [B, L, D+1] — channel D is the 0/1 mask
    u: torch.Tensor,  # [B, H] = (Wq+Wd) q + b1
    Wb: torch.Tensor,  # [H, D] = Wk-Wd
    Wp: torch.Tensor,  # [H, D]
    w2: torch.Tensor,  # [H]
    b2: torch.Tensor,  # []
) -> torch.Tensor:
    """The part of ``act_unit_pool_reference`` the HIP kernels compute
    (csrc/actunit.hip takes the same operands), differentiable in all of
    them.  ``Wb``, ``Wp`` and ``M_b = Wb + Wp * q_b`` are rounded to f16,
    straight-through: the rounding is part of the definition."""
    D = q.shape[-1]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    valid = seq[..., D] != 0
    k = seq[..., :D].to(ct)
    k = torch.where(valid.unsqueeze(-1), k, torch.zeros((), dtype=ct, device=k.device))
    Wb, Wp = _round_f16_st(Wb.to(ct)), _round_f16_st(Wp.to(ct))
    M = _round_f16_st(Wb.unsqueeze(0) + Wp.unsqueeze(0) * q.to(ct).unsqueeze(1))
    h = u.to(ct).unsqueeze(1) + k @ M.transpose(1, 2)  # [B, L, H]
    w = torch.sigmoid(h) @ w2.to(ct) + b2.to(ct)
    w = torch.where(valid, w, torch.zeros((), dtype=ct, device=k.device))
    return (w.unsqueeze(-1) * k).sum(dim=1).to(q.dtype)


def act_unit_pool_reference(
    q: torch.Tensor,  # [B, D]
    seq: torch.Tensor,  # [B, L, D+1] — channel D is the 0/1 mask
    W1: torch.Tensor,  # [H, 4D], column blocks Wq | Wk | Wd | Wp
    b1: torch.Tensor,  # [H]
    w2: torch.Tensor,  # [H]
    b2: torch.Tensor,  # []
) -> torch.Tensor:
    """DIN's local activation unit over a raw slot's tensor, plain torch (not
    in the reference; csrc/actunit.hip is the HIP twin):

        h_l = W1 [q; k_l; q-k_l; q*k_l] + b1
            = u + M k_l,  u = (Wq+Wd) q + b1,  M = (Wk-Wd) + Wp * q
        w_l = <w2, sigmoid(h_l)> + b2
        out = sum_{valid l} w_l * k_l                     -> [B, D], q's dtype

    No softmax: the score is the weight.  The mask selects as in
    ``seq_attn_pool_reference`` (invalid rows are zeros before any
    arithmetic; a sample without a valid cell gives zeros).  Computes in f32
    (f64 for f64 inputs); the f16 roundings of ``M`` and of its two weight
    blocks are straight-through.  Differentiable in everything."""
    D = q.shape[-1]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    Wq, Wk, Wd, Wp = (W1[:, i * D:(i + 1) * D].to(ct) for i in range(4))
    u = torch.addmm(b1.to(ct), q.to(ct), (Wq + Wd).t())
    return act_unit_prepared_reference(q, seq, u, Wk - Wd, Wp, w2, b2)


# ------------------------------------------------- GRU / AUGRU over a raw slot


def seq_gru_reference(
    seq: torch.Tensor,  # [B, L, D+1] — channel D is the 0/1 mask
    Wx: torch.Tensor,  # [3H, D], gates (r, z, n) as nn.GRU's weight_ih_l0
    Wh: torch.Tensor,  # [3H, H], as weight_hh_l0
    bx: torch.Tensor,  # [3H]
    bh: torch.Tensor,  # [3H]
    att: Optional[torch.Tensor] = None,  # [B, L]
    operand_dtype: Optional[torch.dtype] = None,
):
    """GRU (``att`` None: exactly ``torch.nn.GRU`` on the valid rows) or DIEN's
    AUGRU over a raw slot's tensor, plain torch (not in the reference;
    csrc/seqgru.hip is the HIP twin).  With h_{-1} = 0 and x_t = seq[:, t, :D]:

        valid t:   r = sigmoid(Wx_r x + bx_r + Wh_r h + bh_r),  z alike,
                   n = tanh(Wx_n x + bx_n + r * (Wh_n h + bh_n)),
                   h_t = h + a_t (1 - z) (n - h)
        invalid t: h_t = h_{t-1}

    -> (states [B, L, H], last [B, H] = states[:, L-1]) in seq's dtype.  The
    mask selects: invalid rows, and the ``att`` of invalid rows, are replaced
    by zeros before any arithmetic.  Computes in f32 (f64 for f64 inputs); the
    f16 rounding of ``Wx`` and ``Wh`` is part of the definition and
    straight-through, the state is a continuous recurrence.
    ``operand_dtype=torch.float16`` additionally rounds, straight-through, the
    ``h`` that multiplies ``Wh`` and the ``h`` of the update -- the kernels'
    approximation, emulated only to size the tests' bounds."""
    D, H = seq.shape[-1] - 1, Wh.shape[1]
    ct = torch.float64 if seq.dtype == torch.float64 else torch.float32
    zero = torch.zeros((), dtype=ct, device=seq.device)
    valid = seq[..., D] != 0
    x = torch.where(valid.unsqueeze(-1), seq[..., :D].to(ct), zero)
    a = None if att is None else torch.where(valid, att.to(ct), zero)
    Wx, Wh = _round_f16_st(Wx.to(ct)), _round_f16_st(Wh.to(ct))
    gx = x @ Wx.t() + bx.to(ct)  # [B, L, 3H]
    h = torch.zeros(seq.shape[0], H, dtype=ct, device=seq.device)
    states = []
    for t in range(seq.shape[1]):
        hq = _round_f16_st(h) if operand_dtype == torch.float16 else h
        gh = hq @ Wh.t() + bh.to(ct)
        r = torch.sigmoid(gx[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gx[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gx[:, t, 2 * H:] + r * gh[:, 2 * H:])
        step = (1 - z) * (n - hq)
        if a is not None:
            step = a[:, t].unsqueeze(-1) * step
        h = torch.where(valid[:, t].unsqueeze(-1), hq + step, h)
        states.append(h)
    states = torch.stack(states, dim=1).to(seq.dtype)
    return states, states[:, -1]


# ------------------------------------------- self-attention among a raw slot


def seq_self_attn_reference(
    seq: torch.Tensor,  # [B, L, D+1] — channel D is the 0/1 mask
    Wqkv: torch.Tensor,  # [3D, D], rows q | k | v as MultiheadAttention's in_proj_weight
    bqkv: torch.Tensor,  # [3D]
    heads: int,
    causal: bool = False,
    residual: bool = False,
    operand_dtype: Optional[torch.dtype] = None,
) -> torch.Tensor:
    """Multi-head self-attention among the rows of a raw slot's tensor, plain
    torch (not in the reference; csrc/seqsa.hip is the HIP twin).  With x_i =
    seq[:, i, :D], dh = D / heads and W16 = f16(Wqkv):

        valid i:   [q_i | k_i | v_i] = W16 x_i + bqkv
                   s_ij = dh^-1/2 <q_i^h, k_j^h> per head h;  j is allowed for
                   i iff row j is valid and (not causal or j <= i)
                   p_i. = softmax over the allowed j;  o_i^h = sum_j p_ij v_j^h
                   out_i = o_i (+ x_i if residual)
        invalid i: out_i = 0

    -> [B, L, D+1] in seq's dtype with out[..., D] = seq[..., D], a raw-slot
    tensor again.  The mask selects: invalid rows are replaced by zeros before
    any arithmetic and their keys are never allowed, so an Inf or NaN there
    reaches neither an output nor a gradient; a valid row always allows
    itself.  Computes in f32 (f64 for f64 inputs); the f16 rounding of
    ``Wqkv`` is part of the definition and straight-through.
    ``operand_dtype=torch.float16`` additionally rounds, straight-through, q,
    k, v after the projection and p before ``PV`` -- the kernels' MFMA
    operands, emulated only to size the tests' bounds."""
    B, L, D = seq.shape[0], seq.shape[1], seq.shape[2] - 1
    dh = D // heads
    ct = torch.float64 if seq.dtype == torch.float64 else torch.float32
    zero = torch.zeros((), dtype=ct, device=seq.device)
    valid = seq[..., D] != 0
    x = torch.where(valid.unsqueeze(-1), seq[..., :D].to(ct), zero)
    rnd = _round_f16_st if operand_dtype == torch.float16 else (lambda t: t)
    qkv = rnd(x @ _round_f16_st(Wqkv.to(ct)).t() + bqkv.to(ct))
    q, k, v = (t.reshape(B, L, heads, dh).transpose(1, 2)
               for t in qkv.split(D, dim=-1))  # [B, heads, L, dh]
    allowed = valid.unsqueeze(1).expand(B, L, L)  # [B, i, j]
    if causal:
        allowed = allowed & torch.ones(L, L, dtype=torch.bool,
                                       device=seq.device).tril()
    allowed = allowed.unsqueeze(1)
    s = (q @ k.transpose(2, 3)) * float(dh) ** -0.5
    s = s.masked_fill(~allowed, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    den = e.sum(dim=-1, keepdim=True)
    p = rnd(e / torch.where(den > 0, den, torch.ones_like(den)))
    o = (p @ v).transpose(1, 2).reshape(B, L, D)
    if residual:
        o = o + x
    o = torch.where(valid.unsqueeze(-1), o, zero)
    return torch.cat([o.to(seq.dtype), seq[..., D:].detach()], dim=-1)


# ------------------------- the tail of a transformer block over a raw slot


def _layer_norm(v, g, b, eps):
    mean = v.mean(dim=-1, keepdim=True)
    c = v - mean
    return c / torch.sqrt((c * c).mean(dim=-1, keepdim=True) + eps) * g + b


def seq_ffn_reference(
    x: torch.Tensor,  # [B, L, D+1] — the block input, channel D the 0/1 mask
    a: torch.Tensor,  # [B, L, D+1] — the attention output (its mask is ignored)
    Wo: torch.Tensor,  # [D, D]
    bo: torch.Tensor,  # [D]
    g1: torch.Tensor,  # [D]
    be1: torch.Tensor,  # [D]
    W1: torch.Tensor,  # [F, D]
    b1: torch.Tensor,  # [F]
    W2: torch.Tensor,  # [D, F]
    b2: torch.Tensor,  # [D]
    g2: torch.Tensor,  # [D]
    be2: torch.Tensor,  # [D]
    eps: float = 1e-5,
    operand_dtype: Optional[torch.dtype] = None,
) -> torch.Tensor:
    """Out-projection, add & LayerNorm, feed-forward, add & LayerNorm over the
    rows of a raw slot's tensor -- what follows the attention in a post-norm
    ``nn.TransformerEncoderLayer`` with ReLU and no dropout -- in plain torch
    (not in the reference; csrc/seqffn.hip is the HIP twin).  With Wo16, W1_16,
    W2_16 the f16 roundings of the matrices:

        valid i:   u_i = LN(x_i + Wo16 a_i + bo; g1, be1)
                   h_i = relu(W1_16 u_i + b1)
                   y_i = LN(u_i + W2_16 h_i + b2; g2, be2)
        invalid i: out_i = 0

    -> [B, L, D+1] in x's dtype with out[..., D] = x[..., D].  LN is over the D
    channels with the biased variance and ``eps`` inside the square root.  The
    mask of ``x`` selects: invalid rows of ``x`` and ``a`` are replaced by
    zeros before any arithmetic and their outputs by zeros after it.  Computes
    in f32 (f64 for f64 inputs); the f16 rounding of the matrices is part of
    the definition and straight-through.  ``operand_dtype=torch.float16``
    additionally rounds, straight-through, the ``u`` that multiplies ``W1`` and
    the ``h`` that multiplies ``W2`` -- the kernels' MFMA operands, emulated
    only to size the tests' bounds."""
    D = x.shape[-1] - 1
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    zero = torch.zeros((), dtype=ct, device=x.device)
    valid = (x[..., D] != 0).unsqueeze(-1)
    xv = torch.where(valid, x[..., :D].to(ct), zero)
    av = torch.where(valid, a[..., :D].to(ct), zero)
    rnd = _round_f16_st if operand_dtype == torch.float16 else (lambda t: t)
    Wo, W1, W2 = (_round_f16_st(w.to(ct)) for w in (Wo, W1, W2))
    u = _layer_norm(xv + av @ Wo.t() + bo.to(ct), g1.to(ct), be1.to(ct), eps)
    h = torch.relu(rnd(u) @ W1.t() + b1.to(ct))
    y = _layer_norm(u + rnd(h) @ W2.t() + b2.to(ct), g2.to(ct), be2.to(ct), eps)
    y = torch.where(valid, y, zero)
    return torch.cat([y.to(x.dtype), x[..., D:].detach()], dim=-1)


# ------------------------------------------ the DCN-v2 low-rank cross stack


def cross_stack_reference(x0, Vs, Us, bs):
    """A stack of DCN-v2 low-rank cross layers in plain torch (the HIP twin is
    csrc/cross.hip): with x_0 = x0 [B, D], V_l [r, D], U_l [D, r], b_l [D],

        x_{l+1} = x0 * (x_l V_l^T U_l^T + b_l) + x_l

    -> x_n, in the tensors' dtype, differentiable in every argument."""
    xl = x0
    for V, U, b in zip(Vs, Us, bs):
        xl = x0 * (xl @ V.t() @ U.t() + b) + xl
    return xl
