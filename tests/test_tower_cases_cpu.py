"""Models, bounds and case generators of tests/test_gpu_tower_exact.py, and the
checks of them that need no GPU.

The fused DLRM and DCN-v2 towers are assembled in Python (ops/dense.py,
models/dlrm.py, models/dcn.py) from kernels that test_gpu_dense_exact.py pins
one by one.  This file holds what pins the assembly:

* **f64 twins** `dlrm_f64` and `dcn_f64`: the towers written out as plain
  functions of tensors, forward AND backward by hand (no autograd), from the
  models' definitions.  DLRM: bottom MLP (ReLU after every layer), pairwise
  dots of [bottom output, slot 0, slot 1, ...] over the strict lower triangle
  in `tril_indices` order, top MLP on cat([bottom output, dots]), 1-logit
  head.  DCN-v2: x0 = cat([dense, slots, zero pad]), x_{l+1} = x0 * (U(V x_l)
  + b) + x_l (or a full-rank W), deep tower on x0, head on cat([x_L, deep]).
  The packed embedding input is slot-major [S*B, D].  Both end in the mean of
  max(z,0) - z*y + log1p(exp(-|z|)).  They return logits, loss and the
  gradient of every parameter, of the dense input and of the embedding input.
* **stage models**: the f64 result and the per-element bound of one stage from
  the stage's actual input bits -- a fused linear layer (forward, dx, dw, db),
  the packed interaction, the two bf16 roundings of a cross layer, the bf16
  sum of two gradients.  Bounds are those of test_gpu_dense_exact.py's
  docstring (imported, not copied); nothing here is an atol.
* **a tape** (module forward and full-backward hooks) that records every
  stage's input, output, incoming and produced gradient.
* **the BCE model** of csrc/dense.hip bce_fwd / bce_bwd (see `bce_model`).

CPU checks (this file's tests):

* the DLRM twin against the eager module cast to f64: every tensor agrees to
  e = |T - T64|_2 / |T64|_2 <= 2^-40 end to end (measured: bit-equal but for
  the embedding gradient at 4.7e-17), and every stage fed the module's own
  captured input is within (n+1) * 2^-52 * S (measured worst err/bound 0.17);
* the DCN twin against the eager f32 module, stage by stage on the module's
  captured stage inputs, within the f32 accumulation bound (n+1) * 2^-23 * S
  (measured worst err/bound 0.25 for the products; the two single-rounding
  elementwise stages of a cross layer reach 0.998 of their half-ulp bounds),
  and the padded parameter layout against the unpadded one;
* the stage models against a plain torch composition (f32 accumulate, one
  rounding) of the same stage: all ratios <= 1, the bf16 stores reach 0.98;
* the BCE model against an f32 torch evaluation of the kernel's formula.

Wrong variants (`test_wrong_variants_break_the_gate`).  Each wrong twin W is
measured like a tower under test: e_W = |T_W - T64| / |T64| per tensor against
the correct twin, next to e_eager of the eager tower (DLRM: bf16 on CPU; DCN:
f32, the module's CPU compute dtype), and the whole-tower gate of the GPU test
e <= 2 * max(e_eager, 2^-8).  Measured worst e_W / gate over the tensors:

    dlrm  two slots of the base swapped          105
    dlrm  pair order transposed (upper triangle) 74.6
    dlrm  1/B dropped from the loss gradient     2.55e+04
    dcn   pad before the features                212
    dcn   head column blocks not moved           166
    (eager towers themselves                     <= 0.5 by construction)

so every variant lands more than 70 gates out; the test asks for >= 8.
"""
import functools

import pytest
import torch

from test_gpu_dense_exact import (EPS32, REL_BF16, U24, _interact_reference,
                                  acc_bound, bf16_store_bound, colsum_bound,
                                  f16_store_bound)

EPS64 = 2.0 ** -52       # one f64 ulp, relative
MINN32 = 2.0 ** -126     # smallest normal f32 (flush-to-zero floor)
TINY32 = 2.0 ** -150     # half the spacing of f32 subnormals
GATE_FLOOR = 2.0 ** -8   # one bf16 rounding

# v_exp_f32 / v_log_f32 behind __expf / __logf, in f32 ulps (2^-23 relative).
# Not taken from a document but measured on an MI355X, two ways:
#  * the two instructions themselves (exp2 / log2 builtins in a one-off probe
#    kernel) against f64 exp2 / log2: exp2 over 2^23 arguments in [-100, 100]
#    with a normal result, worst 0.694 ulp; log2 over every f32 in [1, 2), the
#    only range bce_fwd_kernel feeds it, worst 0.966 ulp (relative to the
#    result; 0.9985 * 2^-24 absolute);
#  * bce_fwd itself against the f64 reference on 400001 z in [-100, 100] (sig)
#    and 4001 single-element launches (loss term): the derived terms of
#    bce_terms_bound alone already cover every point (least constants that
#    meet the bound: 0 and 0; worst total error of sig 0.923 ulp for |z| < 1
#    and 31.9 ulp at z = -82.5, where the argument product dominates).
# The constants are twice the instruction figures.
EXP_ULPS_MEASURED = 0.694
LOG_ULPS_MEASURED = 0.966
EXP_ULPS = 2 * EXP_ULPS_MEASURED
LOG_ULPS = 2 * LOG_ULPS_MEASURED


# ---------------------------------------------------------------- f64 stages
def _d(t):
    return None if t is None else t.detach().double()


def lin_fwd64(x, W, b):
    """-> (x @ W^T + b, the same from absolute values), no activation."""
    x, W = _d(x), _d(W)
    ref, S = x @ W.t(), x.abs() @ W.abs().t()
    if b is not None:
        ref, S = ref + _d(b), S + _d(b).abs()
    return ref, S


def lin_bwd64(gm, x, W):
    """gm: the gradient at the pre-activation (already masked).
    -> {name: (exact, absolute-value sum)} for dx, dw, db."""
    gm, x, W = _d(gm), _d(x), _d(W)
    return {
        "dx": (gm @ W, gm.abs() @ W.abs()),
        "dw": (gm.t() @ x, gm.abs().t() @ x.abs()),
        "db": (gm.sum(0), gm.abs().sum(0)),
    }


def _pairs(F, device, upper=False):
    if upper:
        return torch.triu_indices(F, F, offset=1, device=device)
    return torch.tril_indices(F, F, offset=-1, device=device)


def interact_fwd64(V, upper=False):
    li, lj = _pairs(V.shape[1], V.device, upper)
    Z = V @ V.transpose(1, 2)
    S = V.abs() @ V.abs().transpose(1, 2)
    return Z[:, li, lj], S[:, li, lj]


def interact_bwd64(V, g, upper=False):
    B, F, _ = V.shape
    li, lj = _pairs(F, V.device, upper)
    G = torch.zeros(B, F, F, dtype=torch.float64, device=V.device)
    G[:, li, lj] = g
    G = G + G.transpose(1, 2)
    return G @ V, G.abs() @ V.abs()


def bce64(z, y, keep_1_over_n=True):
    """-> (per-element terms, loss, dloss/dz)."""
    term = z.clamp_min(0) - z * y + torch.log1p(torch.exp(-z.abs()))
    dz = torch.sigmoid(z) - y
    if keep_1_over_n:
        dz = dz / z.numel()
    return term, term.mean(), dz


def _mlp_fwd(x, layers, last_relu):
    """-> activations [x, a1, ...]; a ReLU after every layer but maybe the last."""
    acts = [x]
    for i, (W, b) in enumerate(layers):
        h, _ = lin_fwd64(acts[-1], W, b)
        relu = last_relu or i < len(layers) - 1
        acts.append(h.relu() if relu else h)
    return acts


def _mlp_bwd(g, acts, layers, last_relu):
    """-> (gradient of the input, [(dw, db) per layer])."""
    grads = []
    for i in reversed(range(len(layers))):
        if last_relu or i < len(layers) - 1:
            g = g * (acts[i + 1] > 0)
        r = lin_bwd64(g, acts[i], layers[i][0])
        grads.append((r["dw"][0], r["db"][0]))
        g = r["dx"][0]
    return g, grads[::-1]


# -------------------------------------------------------------------- twins
def _linears(mod):
    """(weight, bias or None) of every Linear-like layer under `mod`, in
    order (nn.Linear, PALinear and FusedLinear alike; a FusedLinear without
    bias carries a zero buffer)."""
    return [(m.weight, getattr(m, "bias", None)) for m in mod.modules()
            if isinstance(getattr(m, "weight", None), torch.Tensor)
            and m.weight.dim() == 2]


def dlrm_params(model):
    return {"bottom": _linears(model.bottom), "top": _linears(model.top)}


def dcn_params(model):
    cross = []
    for c in model.cross:
        if c.w is not None:
            cross.append({"w": _linears(c.w)[0]})
        else:
            cross.append({"v": _linears(c.v)[0], "u": _linears(c.u)[0]})
    return {"cross": cross, "deep": _linears(model.deep),
            "head": _linears(model.head)[0]}


def _cast(layers):
    return [(_d(W), _d(b)) for W, b in layers]


def _slots(dense, emb):
    """-> ([B, S, D] f64, packed?)"""
    B = dense.shape[0]
    if torch.is_tensor(emb):
        S, D = emb.shape[0] // B, emb.shape[1]
        return _d(emb).view(S, B, D).permute(1, 0, 2), True
    return torch.stack([_d(e) for e in emb], dim=1), False


def _slots_back(g, packed):
    """[B, S, D] -> the layout the embeddings came in."""
    if packed:
        B, S, D = g.shape
        return g.permute(1, 0, 2).reshape(S * B, D)
    return [g[:, s] for s in range(g.shape[1])]


def dlrm_f64(params, dense, base_or_list, y, wrong=None):
    """The DLRM tower in f64.  `wrong` selects a deliberately wrong variant:
    "swap_slots", "upper", "no_1_over_B"."""
    bottom, top = _cast(params["bottom"]), _cast(params["top"])
    emb, packed = _slots(dense, base_or_list)
    S = emb.shape[1]
    perm = list(range(S))
    if wrong == "swap_slots":
        perm[0], perm[1] = perm[1], perm[0]
    emb = emb[:, perm]
    upper = wrong == "upper"

    b_acts = _mlp_fwd(_d(dense), bottom, last_relu=True)
    x = b_acts[-1]
    D = x.shape[1]
    V = torch.cat([x.unsqueeze(1), emb], dim=1)          # feature 0 = bottom
    inter, _ = interact_fwd64(V, upper)
    t_acts = _mlp_fwd(torch.cat([x, inter], dim=1), top, last_relu=False)
    logits = t_acts[-1][:, 0]
    _, loss, dz = bce64(logits, _d(y), wrong != "no_1_over_B")

    g, g_top = _mlp_bwd(dz.unsqueeze(1), t_acts, top, last_relu=False)
    dV, _ = interact_bwd64(V, g[:, D:], upper)
    gx = g[:, :D] + dV[:, 0]
    d_dense, g_bottom = _mlp_bwd(gx, b_acts, bottom, last_relu=True)
    d_emb = dV[:, 1:][:, perm]  # a 2-swap is its own inverse
    return {"logits": logits, "loss": loss, "dense": d_dense,
            "emb": _slots_back(d_emb, packed),
            "bottom": g_bottom, "top": g_top}


def dcn_f64(params, dense, base_or_list, y, wrong=None):
    """The DCN-v2 tower in f64 on parameters of the (possibly padded) width
    in_dim = weight.shape[1] of the first deep layer.  `wrong`: "pad_first",
    "no_1_over_B"."""
    deep, head = _cast(params["deep"]), _cast([params["head"]])[0]
    cross = [{k: _cast([v])[0] for k, v in c.items()} for c in params["cross"]]
    emb, packed = _slots(dense, base_or_list)
    B, S, D = emb.shape
    nd = dense.shape[1]
    feats = torch.cat([_d(dense), emb.reshape(B, S * D)], dim=1)
    in_dim = deep[0][0].shape[1]
    pad = in_dim - feats.shape[1]
    zeros = feats.new_zeros(B, pad)
    lo = pad if wrong == "pad_first" else 0
    x0 = torch.cat([zeros, feats] if lo else [feats, zeros], dim=1)

    xs, projs, mids = [x0], [], []
    for c in cross:
        if "w" in c:
            proj, _ = lin_fwd64(xs[-1], *c["w"])
            mids.append(None)
        else:
            mid, _ = lin_fwd64(xs[-1], c["v"][0], c["v"][1])
            proj, _ = lin_fwd64(mid, *c["u"])
            mids.append(mid)
        projs.append(proj)
        xs.append(x0 * proj + xs[-1])
    d_acts = _mlp_fwd(x0, deep, last_relu=True)
    cat = torch.cat([xs[-1], d_acts[-1]], dim=1)
    logits = lin_fwd64(cat, *head)[0][:, 0]
    _, loss, dz = bce64(logits, _d(y), wrong != "no_1_over_B")

    r = lin_bwd64(dz.unsqueeze(1), cat, head[0])
    g_head = (r["dw"][0], r["db"][0])
    gxl, gd = r["dx"][0][:, :in_dim], r["dx"][0][:, in_dim:]
    gx0, g_deep = _mlp_bwd(gd, d_acts, deep, last_relu=True)
    g_cross = [None] * len(cross)
    for l in reversed(range(len(cross))):
        c = cross[l]
        gx0 = gx0 + gxl * projs[l]
        gp = gxl * x0
        if "w" in c:
            r = lin_bwd64(gp, xs[l], c["w"][0])
            g_cross[l] = {"w": (r["dw"][0], r["db"][0])}
        else:
            ru = lin_bwd64(gp, mids[l], c["u"][0])
            r = lin_bwd64(ru["dx"][0], xs[l], c["v"][0])
            g_cross[l] = {"v": (r["dw"][0], None),
                          "u": (ru["dw"][0], ru["db"][0])}
        gxl = gxl + r["dx"][0]
    gx0 = (gx0 + gxl)[:, lo:lo + nd + S * D]
    return {"logits": logits, "loss": loss, "dense": gx0[:, :nd],
            "emb": _slots_back(gx0[:, nd:].reshape(B, S, D), packed),
            "cross": g_cross, "deep": g_deep, "head": g_head}


def flat(res):
    """One {name: tensor} of a twin's (or `module_result`'s) logits and
    gradients, lists of slots concatenated."""
    out = {"logits": res["logits"], "dense": res["dense"]}
    emb = res["emb"]
    out["emb"] = emb if torch.is_tensor(emb) else torch.cat(list(emb), dim=0)
    for tower in ("bottom", "top", "deep"):
        for i, (dw, db) in enumerate(res.get(tower, [])):
            out[f"{tower}.{i}.w"], out[f"{tower}.{i}.b"] = dw, db
    for l, c in enumerate(res.get("cross", [])):
        for k, (dw, db) in c.items():
            out[f"cross.{l}.{k}.w"] = dw
            if db is not None:
                out[f"cross.{l}.{k}.b"] = db
    if "head" in res:
        out["head.w"], out["head.b"] = res["head"]
    return out


def module_result(model, params_of, logits, dense, emb):
    """The same structure as a twin's result, from a module after backward."""
    def g(layers):
        return [(W.grad, None if b is None else b.grad) for W, b in layers]

    p = params_of(model)
    res = {"logits": logits.detach(), "dense": dense.grad,
           "emb": emb.grad if torch.is_tensor(emb) else [e.grad for e in emb]}
    for tower in ("bottom", "top", "deep"):
        if tower in p:
            res[tower] = g(p[tower])
    if "cross" in p:
        res["cross"] = [{k: g([v])[0] for k, v in c.items()} for c in p["cross"]]
        res["head"] = g([p["head"]])[0]
    return res


def rel_err(T, T64):
    """e = |T - T64|_2 / |T64|_2 (0 when both vanish)."""
    T64 = T64.double()
    den = T64.norm().item()
    num = (T.double() - T64).norm().item()
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def rel_errs(res, res64, skip_missing=False):
    a, b = flat(res), flat(res64)
    return {k: rel_err(a[k], b[k]) for k in b
            if not (skip_missing and a.get(k) is None)}


def gate(e_eager):
    return 2.0 * max(e_eager, GATE_FLOOR)


# ------------------------------------------------ the DCN pad mapping (a copy)
def copy_dcn_fused_to_eager(mf, me, head_moved=True):
    """The pad mapping of test_fused_dcn_matches_eager, read the other way:
    the eager parameters are the un-padded blocks of the fused ones (the
    fused model pads BOTH axes that carry the feature width; the head's
    column blocks move with the pad)."""
    in_e, in_p = me.in_dim, mf.in_dim
    pe, pf = list(me.parameters()), list(mf.parameters())
    assert len(pe) == len(pf)
    with torch.no_grad():
        for a, b in zip(pe[:-2], pf[:-2]):
            a.copy_(b[: a.shape[0], : a.shape[1]] if a.dim() == 2
                    else b[: a.shape[0]])
        hw_e, hw_f = pe[-2], pf[-2]
        if head_moved:
            hw_e[:, :in_e].copy_(hw_f[:, :in_e])
            hw_e[:, in_e:].copy_(hw_f[:, in_p:])
        else:  # the wrong variant
            hw_e.copy_(hw_f[:, : hw_e.shape[1]])
        pe[-1].copy_(pf[-1])


def dcn_unpad(res, in_e, in_p):
    """A padded-layout result (flat dict) cut to the eager layout."""
    out = {}
    for k, t in flat(res).items():
        if k == "head.w":
            t = torch.cat([t[:, :in_e], t[:, in_p:]], dim=1)
        elif k.startswith(("cross", "deep")):
            for dim in range(t.dim()):
                if t.shape[dim] == in_p:
                    t = t.narrow(dim, 0, in_e)
        out[k] = t
    return out


# ------------------------------------------------------------------ the tape
class Tape:
    """Forward and full-backward hooks on every Linear-like layer and on the
    named containers: rec[name] = {in, out, gout, gin}."""

    def __init__(self, model, containers=()):
        self.rec, self._handles = {}, []
        for name, m in model.named_modules():
            w = getattr(m, "weight", None)
            if (isinstance(w, torch.Tensor) and w.dim() == 2) or name in containers:
                self._handles += [
                    m.register_forward_hook(functools.partial(self._fwd, name)),
                    m.register_full_backward_hook(functools.partial(self._bwd, name)),
                ]

    def _fwd(self, name, mod, inp, out):
        r = self.rec.setdefault(name, {})
        r["in"] = tuple(t.detach() for t in inp)
        r["out"] = out.detach()

    def _bwd(self, name, mod, gin, gout):
        r = self.rec[name]
        r["gin"] = tuple(None if t is None else t.detach() for t in gin)
        r["gout"] = gout[0].detach()

    def close(self):
        for h in self._handles:
            h.remove()


def grad_fn_names(t):
    """Names of every node of the autograd graph under tensor `t`."""
    seen, names, stack = set(), set(), [t.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack += [f for f, _ in fn.next_functions]
    return names


# -------------------------------------------------------------- stage models
def worst_ratio(got, ref, bound, what, log=None):
    """Worst err/bound, element-wise; asserts it is <= 1 (a NaN fails)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    bad = int((~(err <= bound)).sum().item())
    print(f"{what}: err/bound {ratio:.4g}")
    if log is not None:
        log[what] = max(log.get(what, 0.0), ratio)
    assert bad == 0, f"{what}: {bad} of {err.numel()} elements exceed the " \
                     f"bound, worst err/bound {ratio:.4g}"
    return ratio


def _bf(t):
    return t.detach().to(torch.bfloat16)


def _kp(k):
    return k + (-k) % 128  # ops/dense.py _pad32: the kernel's reduction length


def fused_linear_fwd_model(x, W, bias, relu):
    """FusedLinear forward from the bits it reads: x and W rounded to bf16,
    the f32 bias; f32 accumulation over the padded K, ReLU, one bf16 store.
    An input wider than the weight (pre-padded) contributes its first
    W.shape[1] columns only.  -> (ref, bound)"""
    k = W.shape[1]
    ref, S = lin_fwd64(_bf(x)[:, :k], _bf(W), bias)
    if relu:
        ref = ref.relu()
    return ref, bf16_store_bound(acc_bound(S, _kp(k)), ref)


def fused_linear_bwd_model(g, out, x, W, relu, splitm, w_dtype):
    """FusedLinear backward from the incoming gradient bits `g` (rounded to
    bf16 as the op does) and the saved output `out` (the ReLU mask).
    dx: f32 accumulation over N, bf16 store; dw: f32 accumulation over the M
    rows in `splitm` parts (+ a bf16 store for bf16 weights); db: M f32
    addends into a zeroed accumulator.  -> {name: (ref, bound)}"""
    M, N = g.shape
    k = W.shape[1]
    gm = _bf(g).double()
    if relu:
        gm = gm * (out.double() > 0)
    r = lin_bwd64(gm, _bf(x)[:, :k], _bf(W))
    dx, Sx = r["dx"]
    dw, Sw = r["dw"]
    db, Sb = r["db"]
    Ew = (M + splitm + 1) * EPS32 * Sw
    return {
        "dx": (dx, bf16_store_bound(acc_bound(Sx, N), dx)),
        "dw": (dw, bf16_store_bound(Ew, dw) if w_dtype == torch.bfloat16 else Ew),
        "db": (db, colsum_bound(M + 1, Sb)),
    }


def interact_model(x, emb_bsd, g):
    """The interaction from the bits its kernels read: V = [x, slots rounded
    to bf16], g the bf16 pair gradient.  -> fwd (ref, bound), dV ref, dV
    accumulation bound E (the caller adds the store of its output type)."""
    V = torch.cat([_bf(x).unsqueeze(1), _bf(emb_bsd)], dim=1)
    fwd, fwd_bound, bwd, bwd_E = _interact_reference(V, _bf(g))
    return (fwd, fwd_bound), bwd, bwd_E


def cross_mix_model(x0, proj, xl):
    """x0 * proj + xl as two bf16 elementwise kernels: the product is rounded,
    then the sum.  -> (ref, bound)"""
    p = x0.double() * proj.double()
    ref = p + xl.double()
    return ref, bf16_store_bound(REL_BF16 * p.abs(), ref)


def cross_dproj_model(g, x0):
    """The gradient the projection receives, g * x0: one bf16 rounding."""
    ref = g.double() * x0.double()
    return ref, REL_BF16 * ref.abs()


def grad_sum_model(ref_a, bound_a, b):
    """The bf16 sum autograd forms of a gradient known to `bound_a` around
    `ref_a` and a second gradient given by its bits.  -> (ref, bound)"""
    ref = ref_a + b.double()
    return ref, bf16_store_bound(bound_a, ref)


# ----------------------------------------------------------------- BCE model
def bce_terms_bound(z, y, exp_ulps, log_ulps):
    """Bounds of the kernel's sigmoid and per-element loss term, from its
    arithmetic (csrc/dense.hip bce_fwd_kernel), z and y the f32 bits in f64.

    e = __expf(-t) = v_exp_f32(rn(-t * log2e)): the product's rounding moves
    the exponent by |t| log2e 2^-24 and the f32 constant is off by 0.22 *
    2^-24 relative, together < 2 |t| 2^-24 relative on e; the instruction adds
    exp_ulps * 2^-23; a result below 2^-126 may be flushed (absolute 2^-126).
    sig = 1 / rn(1 + e): the sum and the correctly rounded quotient add 2^-24
    each; d sig / d e = -sig^2, so E_sig = sig^2 E_e + 2 * 2^-24 sig + 2^-126
    with the e-interval's worst slope taken at its upper sig.
    term = fmaxf(z,0) - z*y + __logf(rn(1 + e')), e' = __expf(-|z|) <= 1: the
    sum 1 + e' is in [1, 2] (absolute 2^-24), log has slope <= 1 there, the
    instruction and the multiply by ln2 (rounding + constant) add
    (log_ulps + 2) * 2^-23 relative to the log, and the three f32 operations
    around it 2^-24 each (an fma contraction only removes one).
    -> (sig64, E_sig, term64, E_term)"""
    u = U24
    az = z.abs()
    sig = torch.sigmoid(z)
    term = z.clamp_min(0) - z * y + torch.log1p(torch.exp(-az))

    def exp_err(t):  # relative error of __expf(-t) and the flush floor
        return 2 * t.abs() * u + exp_ulps * EPS32

    # sig: e = exp(-z) may be huge; work with sig = 1/(1+e) directly.  A
    # relative error d on e moves sig by at most sig * (1 - sig) * d / (1 - d)
    d = exp_err(z)
    E_sig = sig * (1 - sig) * d / (1 - d) + 2 * u * sig * (1 + d) + 2 * MINN32
    # term
    e = torch.exp(-az)
    E_e = e * exp_err(az) + MINN32
    E_s = E_e + u * (1 + e + E_e)
    L = torch.log1p(e)
    E_L = E_s + (log_ulps + 2) * EPS32 * (L + E_s)
    zy = (z * y).abs()
    E1 = u * zy
    a = (z.clamp_min(0) - z * y).abs()
    E2 = E1 + u * (a + E1)
    E_term = E2 + E_L + u * (term.abs() + E2 + E_L)
    return sig, E_sig, term, E_term


def bce_model(z, y, g, sig_stored, exp_ulps, log_ulps):
    """-> {loss, sig, dz: (ref, bound)} for n = z.numel() elements.
    loss: the block tree (256 lanes, 8 levels) and one atomic per block add
    (n_blocks + 8) * 2^-24 * sum|terms| / n; the final division one rounding.
    dz = g * (sig_stored - y) / n from the STORED f32 sigmoid: three f32
    roundings, 3 * 2^-24 |ref| (+ 3 * 2^-48 |ref| second order) + 2^-150."""
    z, y, g = z.double(), y.double(), g.double()
    n = z.numel()
    sig, E_sig, term, E_term = bce_terms_bound(z, y, exp_ulps, log_ulps)
    n_blocks = (n + 255) // 256
    tot = (term.abs() + E_term).sum()
    loss = term.sum() / n
    E_loss = (E_term.sum() + (n_blocks + 8) * U24 * tot) / n
    E_loss = E_loss + U24 * (loss.abs() + E_loss)
    dz = g * (sig_stored.double() - y) / n
    E_dz = (3 * U24 + 3 * U24 * U24 + U24 ** 3) * dz.abs() + TINY32
    return {"loss": (loss, E_loss), "sig": (sig, E_sig), "dz": (dz, E_dz)}


def _least(ok, hi):
    """Bisection for the least c in [0, hi] with ok(c) (ok is monotone)."""
    if ok(0.0):
        return 0.0
    lo = 0.0
    for _ in range(50):
        mid = (lo + hi) / 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


def bce_exp_ulps_needed(z, sig):
    """The least exp_ulps at which the kernel's `sig` meets bce_terms_bound."""
    z = z.double()
    y = torch.zeros_like(z)
    err = (sig.double() - torch.sigmoid(z)).abs()
    return _least(lambda c: bool((err <= bce_terms_bound(z, y, c, 0.0)[1]).all()),
                  4096.0)


def bce_log_ulps_needed(z, y, terms, exp_ulps):
    """The least log_ulps at which the kernel's per-element `terms` (n = 1
    launches) meet bce_terms_bound, given exp_ulps."""
    z, y = z.double(), y.double()
    t64 = bce_terms_bound(z, y, 0.0, 0.0)[2]
    err = (terms.double() - t64).abs()
    return _least(
        lambda c: bool((err <= bce_terms_bound(z, y, exp_ulps, c)[3]).all()),
        2.0 ** 30)


BCE_PLANTED = [0.0, 2.0 ** -20, -(2.0 ** -20), 17.0, -17.0, 30.0, -30.0,
               88.0, -88.0, 100.0, -100.0]
BCE_SIZES = (1, 255, 256, 257, 4099)
BCE_SCALES = (1.0, 1024.0, 2.0 ** -10)


def bce_case(n, soft, device, dtype=torch.float32):
    """z = randn * 3 with the planted values at seeded positions (as many as
    fit), labels hard 0/1 or uniform(0, 1)."""
    gen = torch.Generator().manual_seed(1000003 * n + int(soft))
    z = torch.randn(n, generator=gen) * 3
    where = torch.randperm(n, generator=gen)[: len(BCE_PLANTED)]
    z[where] = torch.tensor(BCE_PLANTED[: len(where)])
    y = torch.rand(n, generator=gen)
    if not soft:
        y = (y > 0.5).float()
    return z.to(dtype).to(device), y.to(device)


# ------------------------------------------------------------- tower cases
# name -> (kind, constructor kwargs, B, bf16 module?, embeddings as a list?)
_SMALL = dict(num_sparse=3, num_dense=13, dim=32, bottom_mlp=(64,), top_mlp=(64, 32))
_DCN = dict(num_sparse=3, num_dense=13, dim=32, num_cross=2, deep=(64, 32))
CASES = {
    "dlrm-small": ("dlrm", _SMALL, 200, True, False),
    "dlrm-odd": ("dlrm", dict(num_sparse=16, num_dense=5, dim=64,
                              bottom_mlp=(96,), top_mlp=(96, 64)), 129, True, False),
    "dlrm-bench": ("dlrm", dict(), 256, True, False),
    "dlrm-list": ("dlrm", _SMALL, 200, True, True),
    "dlrm-f32": ("dlrm", _SMALL, 200, False, False),
    "dcn-lowrank": ("dcn", dict(_DCN, cross_rank=32), 200, True, False),
    "dcn-full": ("dcn", dict(_DCN, cross_rank=0), 200, True, False),
    "dcn-nopad": ("dcn", dict(_DCN, num_dense=32, cross_rank=32), 129, True, False),
}


def make_model(name, fused, device, seed=1234):
    """The module's own init under a fixed seed."""
    from persia_amd.models import DCNv2, DLRM

    kind, kw, _, bf16, _ = CASES[name]
    torch.manual_seed(seed)
    m = (DLRM if kind == "dlrm" else DCNv2)(fused=fused, **kw).to(device)
    return m.bfloat16() if bf16 else m


def make_inputs(name, device, as_list=None):
    """Seeded from the shape: dense randn, base (randn * 0.5) f16 slot-major
    [S*B, D] (or the list of its slots), labels 0/1.  All leaves."""
    kind, kw, B, _, lst = CASES[name]
    as_list = lst if as_list is None else as_list
    full = dict(num_sparse=26, num_dense=13, dim=128 if kind == "dlrm" else 64)
    full.update(kw)
    S, nd, D = full["num_sparse"], full["num_dense"], full["dim"]
    seed = 0
    for s in (B, S, nd, D):
        seed = seed * 1000003 + s
    gen = torch.Generator().manual_seed(seed % (2 ** 62))
    dense = torch.randn(B, nd, generator=gen).to(device).requires_grad_(True)
    base = (torch.randn(S * B, D, generator=gen) * 0.5).to(torch.float16).to(device)
    y = (torch.rand(B, generator=gen) > 0.5).float().to(device)
    if as_list:
        emb = [base[s * B:(s + 1) * B].clone().requires_grad_(True)
               for s in range(S)]
    else:
        emb = base.requires_grad_(True)
    return dense, emb, y


# ================================================================ CPU checks
def _run(model, dense, emb, y, containers=()):
    tape = Tape(model, containers)
    logits = model(dense, emb)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(
        logits.float() if logits.dtype == torch.bfloat16 else logits,
        y.to(torch.float32 if logits.dtype == torch.bfloat16 else logits.dtype))
    loss.backward()
    tape.close()
    return tape, logits


def _check_eager_linear(rec, mod, eps, log, name):
    """One eager Linear stage on its captured input: forward, dx, dw, db
    within (n + 1) * eps * S."""
    x, out, g = rec["in"][0], rec["out"], rec["gout"]
    M, K = x.shape
    N = out.shape[1]
    ref, S = lin_fwd64(x, mod.weight, mod.bias)
    worst_ratio(out, ref, (K + 1) * eps * S, f"{name} fwd", log)
    r = lin_bwd64(g, x, mod.weight)
    if rec["gin"][0] is not None:
        worst_ratio(rec["gin"][0], r["dx"][0], (N + 1) * eps * r["dx"][1],
                    f"{name} dx", log)
    worst_ratio(mod.weight.grad, r["dw"][0], (M + 1) * eps * r["dw"][1],
                f"{name} dw", log)
    if mod.bias is not None:
        worst_ratio(mod.bias.grad, r["db"][0], (M + 1) * eps * r["db"][1],
                    f"{name} db", log)


def test_dlrm_twin_matches_eager_f64_module():
    from persia_amd.models import DLRM

    torch.manual_seed(5)
    m = DLRM(fused=False, **_SMALL).double()
    dense, base, y = make_inputs("dlrm-small", "cpu")
    dense = dense.detach().double().requires_grad_(True)
    base = base.detach().double().requires_grad_(True)
    tape, logits = _run(m, dense, base, y.double(), ("interaction", "bottom", "top"))
    twin = dlrm_f64(dlrm_params(m), dense, base, y)
    es = rel_errs(module_result(m, dlrm_params, logits, dense, base), twin)
    print("twin vs f64 module:", {k: f"{v:.2e}" for k, v in es.items()})
    assert max(es.values()) <= 2.0 ** -40, es
    assert abs(twin["loss"].item() - torch.nn.functional.
               binary_cross_entropy_with_logits(logits, y.double()).item()) \
        <= 8 * EPS64

    log = {}
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Linear):
            _check_eager_linear(tape.rec[name], mod, EPS64, log, name)
    # the interaction on the module's own [B, F, D] input; its backward is two
    # batched products and a sum: F + 2 roundings
    rec = tape.rec["interaction"]
    V = rec["in"][0]
    F_, D = V.shape[1], V.shape[2]
    fwd, S = interact_fwd64(V)
    worst_ratio(rec["out"], fwd, (D + 1) * EPS64 * S, "interaction fwd", log)
    dV, SV = interact_bwd64(V, rec["gout"])
    worst_ratio(rec["gin"][0], dV, (F_ + 2) * EPS64 * SV, "interaction dV", log)
    # glue: the top input is cat([bottom out, inter]) bit for bit; the bottom
    # output's gradient is the sum of its two contributions, one rounding
    xb = tape.rec["bottom"]["out"]
    assert torch.equal(tape.rec["top"]["in"][0], torch.cat([xb, rec["out"]], 1))
    gsum = tape.rec["top"]["gin"][0][:, :D] + rec["gin"][0][:, 0]
    worst_ratio(tape.rec["bottom"]["gout"], gsum.double(),
                EPS64 * gsum.abs(), "bottom gout", log)
    print("worst stage err/bound:", max(log.values()))

    # the list form of the embeddings gives the twin the same numbers
    B = dense.shape[0]
    lst = [base.detach()[s * B:(s + 1) * B] for s in range(3)]
    twin_l = dlrm_f64(dlrm_params(m), dense, lst, y)
    assert torch.equal(twin_l["logits"], twin["logits"])
    assert torch.equal(torch.cat(twin_l["emb"], 0), twin["emb"])


def _dcn_pair(rank, num_dense=13):
    """An f32 fused-layout parameter container and its eager f32 twin module."""
    from persia_amd.models import DCNv2

    kw = dict(_DCN, cross_rank=rank, num_dense=num_dense)
    torch.manual_seed(6)
    mf = DCNv2(fused=True, **kw)
    me = DCNv2(fused=False, **kw)
    copy_dcn_fused_to_eager(mf, me)
    return mf, me


@pytest.mark.parametrize("rank", [32, 0], ids=["lowrank", "full"])
def test_dcn_twin_matches_eager_f32_module_stage_by_stage(rank):
    mf, me = _dcn_pair(rank)
    dense, base, y = make_inputs("dcn-lowrank", "cpu")
    base = base.detach().float().requires_grad_(True)  # no f16 store of its grad
    names = tuple(f"cross.{l}" for l in range(len(me.cross)))
    tape, logits = _run(me, dense, base, y, names)
    log = {}
    for name, mod in me.named_modules():
        if isinstance(mod, torch.nn.Linear):
            _check_eager_linear(tape.rec[name], mod, EPS32, log, name)
    for l, name in enumerate(names):
        rec, c = tape.rec[name], me.cross[l]
        x0, xl = rec["in"]
        proj = tape.rec[name + (".w" if c.w is not None else ".u")]
        p = x0.double() * proj["out"].double()
        ref = p + xl.double()
        worst_ratio(rec["out"], ref, U24 * p.abs() + U24 * (ref.abs() + U24 * p.abs()),
                    f"{name} mix", log)
        gp = rec["gout"].double() * x0.double()
        worst_ratio(proj["gout"], gp, U24 * gp.abs(), f"{name} dproj", log)
    print("worst stage err/bound:", max(log.values()))

    # end to end: the twin on the eager parameters and on the padded layout
    t_e = dcn_f64(dcn_params(me), dense, base, y)
    t_p = dcn_f64(dcn_params(mf), dense, base, y)
    got = module_result(me, dcn_params, logits, dense, base)
    es = rel_errs(got, t_e, skip_missing=True)
    print("eager f32 vs twin:", {k: f"{v:.2e}" for k, v in es.items()})
    assert max(es.values()) <= 2.0 ** -16, es  # f32 tower against f64
    cut, fe = dcn_unpad(t_p, me.in_dim, mf.in_dim), flat(t_e)
    for k, t in fe.items():
        if t is not None:
            assert rel_err(cut[k], t) <= 2.0 ** -40, k
    # and what multiplies a pad feature has an exactly zero gradient
    fp = flat(t_p)
    in_e = me.in_dim
    assert mf.pad == 19
    assert (fp["deep.0.w"][:, in_e:] == 0).all()
    assert (fp["head.w"][:, in_e:mf.in_dim] == 0).all()


def test_stage_models_hold_for_a_plain_composition():
    """An f32-accumulating torch composition of each stage, with one rounding
    per store, stays inside the stage models' bounds (and the bf16 store
    term is reached: the bounds are not slack)."""
    gen = torch.Generator().manual_seed(11)
    M, K, N = 200, 38, 64
    x = (torch.randn(M, K, generator=gen) * 0.5).to(torch.bfloat16)
    xp = torch.nn.functional.pad(x, (0, 90))  # arrives pre-padded
    W = torch.randn(N, K, generator=gen) * 0.25 + 0.05
    b = torch.randn(N, generator=gen)
    g = (torch.randn(M, N, generator=gen) * 0.5).to(torch.bfloat16)
    Wb = W.to(torch.bfloat16)
    log = {}
    for relu in (True, False):
        pre = x.float() @ Wb.float().t() + b
        out = (pre.relu() if relu else pre).to(torch.bfloat16)
        for xin in (x, xp):
            ref, bound = fused_linear_fwd_model(xin, W, b, relu)
            worst_ratio(out, ref, bound, f"fwd relu={relu}", log)
        gm = g.float() * (out > 0) if relu else g.float()
        for wd in (torch.float32, torch.bfloat16):
            mdl = fused_linear_bwd_model(g, out, xp, W, relu, 2, wd)
            worst_ratio((gm @ Wb.float()).to(torch.bfloat16), *mdl["dx"], "dx", log)
            worst_ratio((gm.t() @ x.float()).to(wd), *mdl["dw"], f"dw {wd}", log)
            worst_ratio(gm.sum(0), *mdl["db"], "db", log)
    assert log["fwd relu=True"] > 0.5 and log["dx"] > 0.5

    B, S, D = 33, 3, 32
    xb = (torch.randn(B, D, generator=gen) * 0.5).to(torch.bfloat16)
    emb = (torch.randn(B, S, D, generator=gen) * 0.5).to(torch.float16)
    gi = (torch.randn(B, 6, generator=gen) * 0.5).to(torch.bfloat16)
    (fwd, fb), dV, E = interact_model(xb, emb, gi)
    V = torch.cat([xb.unsqueeze(1), emb.to(torch.bfloat16)], 1).float()
    li, lj = torch.tril_indices(4, 4, offset=-1)
    worst_ratio((V @ V.transpose(1, 2))[:, li, lj].to(torch.bfloat16), fwd, fb,
                "interact fwd", log)
    G = torch.zeros(B, 4, 4)
    G[:, li, lj] = gi.float()
    got = (G + G.transpose(1, 2)) @ V
    worst_ratio(got[:, 1:].to(torch.float16), dV[:, 1:],
                f16_store_bound(E[:, 1:], dV[:, 1:]), "interact dbase", log)
    # the sum of the two gradients of the bottom output
    other = (torch.randn(B, D, generator=gen) * 0.5).to(torch.bfloat16)
    dx_i = got[:, 0].to(torch.bfloat16)
    ref, bound = grad_sum_model(dV[:, 0], bf16_store_bound(E[:, 0], dV[:, 0]), other)
    worst_ratio(dx_i + other, ref, bound, "grad sum", log)
    # the cross layer's two roundings
    x0, pr, xl = xb, other, (torch.randn(B, D, generator=gen)).to(torch.bfloat16)
    worst_ratio(x0 * pr + xl, *cross_mix_model(x0, pr, xl), "cross mix", log)
    worst_ratio(xl * x0, *cross_dproj_model(xl, x0), "cross dproj", log)
    # a swapped slot pair is far outside the interaction bound
    err = ((V[:, [0, 2, 1, 3]] @ V[:, [0, 2, 1, 3]].transpose(1, 2))[:, li, lj]
           .double() - fwd).abs()
    assert (err / fb).max().item() > 100


def _variant_factors():
    from persia_amd.models import DLRM

    out = {}
    # ---- DLRM: the eager bf16 tower as the "kernel"
    torch.manual_seed(1234)
    m = DLRM(fused=False, **_SMALL).bfloat16()
    dense, base, y = make_inputs("dlrm-small", "cpu")
    _, logits = _run(m, dense, base, y)
    p = dlrm_params(m)
    good = dlrm_f64(p, dense, base, y)
    e_eager = rel_errs(module_result(m, dlrm_params, logits, dense, base), good)
    gates = {k: gate(v) for k, v in e_eager.items()}
    out["dlrm eager"] = max(e_eager[k] / gates[k] for k in gates)
    for wrong in ("swap_slots", "upper", "no_1_over_B"):
        e = rel_errs(dlrm_f64(p, dense, base, y, wrong=wrong), good)
        out["dlrm " + wrong] = max(e[k] / gates[k] for k in gates)
    # ---- DCN: the eager f32 tower (the module's CPU compute dtype)
    mf, me = _dcn_pair(32)
    dense, base, y = make_inputs("dcn-lowrank", "cpu")
    base = base.detach().float().requires_grad_(True)
    _, logits = _run(me, dense, base, y)
    good = dcn_f64(dcn_params(mf), dense, base, y)
    cut = dcn_unpad(good, me.in_dim, mf.in_dim)
    got = flat(module_result(me, dcn_params, logits, dense, base))
    gates = {k: gate(rel_err(got[k], cut[k])) for k in cut if got[k] is not None}
    out["dcn eager"] = max(rel_err(got[k], cut[k]) / gates[k] for k in gates)
    bad = dcn_unpad(dcn_f64(dcn_params(mf), dense, base, y, wrong="pad_first"),
                    me.in_dim, mf.in_dim)
    out["dcn pad_first"] = max(rel_err(bad[k], cut[k]) / gates[k] for k in gates)
    # head blocks not moved: the eager parameters taken from the wrong columns
    _, me_bad = _dcn_pair(32)
    copy_dcn_fused_to_eager(mf, me_bad, head_moved=False)
    bad = flat(dcn_f64(dcn_params(me_bad), dense, base, y))
    out["dcn head_not_moved"] = max(rel_err(bad[k], cut[k]) / gates[k]
                                    for k in gates)
    return out


def test_wrong_variants_break_the_gate():
    f = _variant_factors()
    print({k: f"{v:.3g}" for k, v in f.items()})
    assert f.pop("dlrm eager") <= 0.5 and f.pop("dcn eager") <= 0.5
    assert len(f) == 5
    for k, v in f.items():
        assert v >= 8, (k, v)


def _f32_bce(z, y, g):
    """The kernel's formula evaluated in f32 by torch (libm exp / log)."""
    n = z.numel()
    sig = 1.0 / (1.0 + torch.exp(-z))
    term = z.clamp_min(0) - z * y + torch.log(1.0 + torch.exp(-z.abs()))
    loss = term.sum() / n
    return loss, sig, g * (sig - y) / n


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("n", BCE_SIZES)
def test_bce_model_holds_for_f32_torch(n, soft):
    """libm's expf / logf are within 1 ulp, so the model must hold for torch's
    f32 evaluation with exp_ulps = log_ulps = 1 -- and break when 1/n is
    dropped from dz or sigmoid(-z) is stored."""
    z, y = bce_case(n, soft, "cpu")
    assert (z == 100).any() or n < len(BCE_PLANTED)
    for scale in BCE_SCALES:
        g = torch.tensor(scale)
        loss, sig, dz = _f32_bce(z, y, g)
        mdl = bce_model(z, y, g, sig, 1.0, 1.0)
        worst_ratio(loss, *mdl["loss"], f"loss n={n}")
        worst_ratio(sig, *mdl["sig"], f"sig n={n}")
        worst_ratio(dz, *mdl["dz"], f"dz n={n} scale={scale}")
        assert torch.isfinite(loss) and torch.isfinite(dz).all()
        if n > 1:
            ref, bound = mdl["dz"]
            assert ((dz.double() * n - ref).abs() > bound).any()
            ref, bound = mdl["sig"]
            assert ((1 - sig.double() - ref).abs() > bound).any()
    need = bce_exp_ulps_needed(z, sig)
    assert need <= 1.0, need
