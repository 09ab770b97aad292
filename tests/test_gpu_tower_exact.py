"""The fused DLRM and DCN-v2 towers as assembled, and the BCE kernels, against
the f64 models of test_tower_cases_cpu.py.

a. Teacher-forced stage chain.  Every stage of a tower is held element-wise
   to its stage model evaluated on the bits the stage actually received
   (module forward / full-backward hooks, hooks on `bottom`, `top`, `deep`
   and the cross layers, `.grad` of the leaves).  FusedMLP's backward chain
   (FusedChainFn) never calls its layers' forward, so its interior is read
   from a second run with PA_FUSED_DRELU=0 (one FusedLinearFn per layer):
   the chained run must reproduce that run's logits, boundary gradients and
   leaf gradients bit for bit, and its parameter gradients must meet the
   stage models built from the per-layer run's bits.
b. Whole-tower net: e = |T - T64|_2 / |T64|_2 of the logits and of every
   gradient against the twin, for the fused tower and for the eager bf16
   tower with the same parameter bits; gate e_fused <= 2 * max(e_eager, 2^-8).
c. Exact structure: zero gradients of everything that multiplies a DCN pad
   feature, before and after an SGD step; packed base == list of slots.
d. Negative control: two slots of the base swapped break the interaction
   bound.
e. bce_fwd / bce_bwd against bce_model.

Measured on an MI355X (worst err/bound per stage kind over all cases; every
bound as derived, none raised):

  stage                                   worst err/bound
  fused linear forward (bf16 store)       0.986
  fused linear dx (bf16 store)            0.992
  fused linear dw, bf16 weights           0.982   (chain == per-layer)
  fused linear dw, f32 weights / slots    0.0021 / 0.0019
  fused linear db (f32 column sums)       0.0018
  interaction forward                     0.987
  base.grad (f16 store)                   0.998   (list of slots: 0.988)
  bottom output gradient (bf16 sum)       0.963
  cross layer x0 * proj + xl              0.983
  cross layer g * x0                      0.988
  (the 0.95 .. 0.99 rows are one bf16 / f16 store: tight by construction)

Whole-tower net, e_fused / e_eager (range over the gradient tensors) and the
worst e_fused / gate; the two towers share their dominant roundings (bf16
logits, bf16 dz), hence the near-equal pairs; the factor 2 was never needed
(worst e_fused / e_eager 1.007):

  case         logits             gradients e_fused      e_eager              /gate
  dlrm-small   3.94e-3 / 3.94e-3  6.64e-3 .. 1.08e-1     6.64e-3 .. 1.08e-1   0.502
  dlrm-odd     4.27e-3 / 4.27e-3  3.81e-3 .. 8.36e-2     3.81e-3 .. 8.34e-2   0.502
  dlrm-bench   5.63e-3 / 5.63e-3  1.81e-4 .. 1.28e-1     1.81e-4 .. 1.28e-1   0.500
  dlrm-list    3.94e-3 / 3.94e-3  6.64e-3 .. 1.08e-1     6.64e-3 .. 1.08e-1   0.502
  dlrm-f32     4.09e-3 / 4.34e-3  3.17e-3 .. 1.22e-1     8.15e-3 .. 1.23e-1   0.502
  dcn-lowrank  3.10e-3 / 3.10e-3  2.65e-3 .. 2.95e-2     3.14e-3 .. 2.96e-2   0.500
  dcn-full     3.20e-3 / 3.20e-3  5.95e-4 .. 4.15e-2     5.95e-4 .. 4.20e-2   0.503
  dcn-nopad    3.30e-3 / 3.30e-3  3.12e-3 .. 7.27e-2     3.68e-3 .. 7.26e-2   0.504

BCE (constants EXP_ULPS = 2 * 0.694, LOG_ULPS = 2 * 0.966, measured as the
comment at their definition says): worst err/bound loss 0.149, sig 0.702,
dz 0.964 (three half-ulp roundings), per-element term on the sweep 0.554;
the sweep needs 0 of the exp constant.

Two things the issue states differently, both for a reason in the kernels:
weight and bias gradients of the packed and the list run are split-M atomic
sums (4 parts at M = 200), so they are held to the stage bounds, not to bit
equality (dcn-full's first cross weight differed in the first run); and the
loss of two calls is bit-equal only up to two blocks, beyond that equal to
within the reordering bound of its n_blocks atomics.
"""
import functools
import os

import pytest
import torch

import test_tower_cases_cpu as T
from test_gpu_dense_exact import (_bits, _parse_wgrad_config, bf16_store_bound,
                                  f16_store_bound)

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _native():
    from persia_amd.ops import native

    return native()


# ------------------------------------------------------------------- running
def _fused_layers(model):
    from persia_amd.ops.dense import FusedLinear

    return [(n, m) for n, m in model.named_modules() if isinstance(m, FusedLinear)]


def _containers(model, kind):
    if kind == "dlrm":
        return ("bottom", "top")
    return ("deep",) + tuple(f"cross.{l}" for l in range(len(model.cross)))


def _swap_slots(base, B):
    out = base.detach().clone()
    out[:B], out[B:2 * B] = base.detach()[B:2 * B], base.detach()[:B]
    return out.requires_grad_(True)


def _run_fused(name, per_layer=False, side=False, as_list=None, swap=False,
               backwards=1):
    """One forward + backward of the fused tower of case `name`."""
    from persia_amd.ops.dense import fused_bce_with_logits

    kind, _, B, _, _ = T.CASES[name]
    model = T.make_model(name, True, _dev())
    dense, emb, y = T.make_inputs(name, _dev(), as_list)
    if swap:
        emb = _swap_slots(emb, B)
    slots = {}
    if side:
        for n, m in _fused_layers(model):
            for p in (m.weight, m.bias):
                p._sideband_grad = torch.zeros_like(p, dtype=torch.float32)
            slots[n] = (m.weight._sideband_grad, m.bias._sideband_grad)
    old = os.environ.get("PA_FUSED_DRELU")
    os.environ["PA_FUSED_DRELU"] = "0" if per_layer else "1"
    try:
        for _ in range(backwards):
            tape = T.Tape(model, _containers(model, kind))
            logits = model(dense, emb)
            names = T.grad_fn_names(logits)
            fused_bce_with_logits(logits, y).backward()
            tape.close()
    finally:
        if old is None:
            del os.environ["PA_FUSED_DRELU"]
        else:
            os.environ["PA_FUSED_DRELU"] = old
    torch.cuda.synchronize()
    return dict(model=model, tape=tape, logits=logits.detach(), dense=dense,
                emb=emb, y=y, names=names, slots=slots, kind=kind)


@functools.lru_cache(maxsize=None)
def _chain(name):
    return _run_fused(name)


@functools.lru_cache(maxsize=None)
def _layered(name):
    return _run_fused(name, per_layer=True)


def _assert_paths(name, run, per_layer):
    """The path under test was really taken."""
    kind, kw, _, _, lst = T.CASES[name]
    names = run["names"]
    if per_layer:
        assert "FusedLinearFnBackward" in names
        assert "FusedChainFnBackward" not in names
    else:
        assert "FusedChainFnBackward" in names
    if kind == "dlrm":
        m = run["model"]
        assert _native().interact_packed_feasible(m.num_sparse + 1, m.dim)
        want = "_InteractFnBackward" if lst else "_InteractPackedFnBackward"
        assert want in names, names


# ------------------------------------------------------------ a. stage chain
def _layer_models(name):
    """Stage checks of every fused layer on the per-layer run's captured
    bits.  -> ({layer: backward model}, log of worst ratios)"""
    run = _layered(name)
    C = _native()
    log, models = {}, {}
    for n, mod in _fused_layers(run["model"]):
        rec = run["tape"].rec[n]
        x, out, g = rec["in"][0], rec["out"], rec["gout"]
        M, N, k = x.shape[0], out.shape[1], mod.weight.shape[1]
        assert out.dtype == torch.bfloat16
        T.worst_ratio(out, *T.fused_linear_fwd_model(x, mod.weight, mod.bias,
                                                     mod.relu), f"{n} fwd", log)
        assert (x[:, k:] == 0).all()  # a pre-padded input's tail
        _, splitm, _ = _parse_wgrad_config(C.wgrad_config(M, N, T._kp(x.shape[1])))
        for wd in (mod.weight.dtype, torch.float32):
            models[(n, wd)] = T.fused_linear_bwd_model(
                g, out, x, mod.weight, mod.relu, splitm, wd)
        dx = rec["gin"][0]
        assert dx is not None and dx.shape == x.shape
        T.worst_ratio(dx[:, :k], *models[(n, torch.float32)]["dx"], f"{n} dx", log)
        assert (dx[:, k:] == 0).all()
    return models, log


def _check_param_grads(models, layers, grads_of, log, tag, f32=False, scale=1):
    for n, mod in layers:
        dw, db = grads_of(n, mod)
        mdl = models[(n, torch.float32 if f32 else mod.weight.dtype)]
        assert dw.shape == mod.weight.shape
        f = scale * scale  # n and sum|a| both scale
        T.worst_ratio(dw, scale * mdl["dw"][0], f * mdl["dw"][1],
                      f"{n} dw {tag}", log)
        if db is not None:
            assert db.shape == mod.bias.shape and db.dtype == torch.float32
            T.worst_ratio(db, scale * mdl["db"][0], f * mdl["db"][1],
                          f"{n} db {tag}", log)


def _module_grads(n, mod):
    return mod.weight.grad, mod.bias.grad  # bias.grad None: a buffer


def _emb_bsd(run):
    dense, emb = run["dense"], run["emb"]
    B = dense.shape[0]
    if torch.is_tensor(emb):
        return emb.detach().view(-1, B, emb.shape[1]).permute(1, 0, 2)
    return torch.stack([e.detach() for e in emb], dim=1)


def _check_dlrm_glue(run, log, emb_bsd=None, only_inter=False):
    """The assembly around the interaction, from captured neighbours."""
    rec = run["tape"].rec
    m = run["model"]
    xb, top_in, gtop = rec["bottom"]["out"], rec["top"]["in"][0], rec["top"]["gin"][0]
    B, D = xb.shape
    F_ = m.num_sparse + 1
    P = F_ * (F_ - 1) // 2
    packed = torch.is_tensor(run["emb"])
    width = T._kp(D + P) if packed else D + P
    assert top_in.shape == (B, width) and gtop.shape == (B, width)
    inter = top_in[:, D:D + P]
    # top input == cat([bottom out, inter, zeros]) bit for bit
    assert torch.equal(_bits(top_in),
                       _bits(torch.cat([xb, inter, xb.new_zeros(B, width - D - P)], 1)))
    emb = _emb_bsd(run) if emb_bsd is None else emb_bsd
    (fwd, fb), dV, E = T.interact_model(xb, emb, gtop[:, D:D + P])
    T.worst_ratio(inter, fwd, fb, "interaction fwd", log)
    if only_inter:
        return
    assert (gtop[:, D + P:] == 0).all()  # zero weight columns: zero dx there
    if packed:
        ref = dV[:, 1:].permute(1, 0, 2).reshape(-1, D)
        Eb = E[:, 1:].permute(1, 0, 2).reshape(-1, D)
        assert run["emb"].grad.dtype == torch.float16
        T.worst_ratio(run["emb"].grad, ref, f16_store_bound(Eb, ref), "dbase", log)
    else:
        for s, e in enumerate(run["emb"]):
            ref = dV[:, 1 + s]
            T.worst_ratio(e.grad, ref,
                          f16_store_bound(bf16_store_bound(E[:, 1 + s], ref), ref),
                          "dbase (list)", log)
    ref, bound = T.grad_sum_model(dV[:, 0], bf16_store_bound(E[:, 0], dV[:, 0]),
                                  gtop[:, :D])
    T.worst_ratio(rec["bottom"]["gout"], ref, bound, "bottom gout (sum)", log)


def _check_dcn_glue(run, log):
    rec, m = run["tape"].rec, run["model"]
    dense = run["dense"].detach()
    B = dense.shape[0]
    feats = torch.cat([dense.to(torch.bfloat16),
                       _emb_bsd(run).reshape(B, -1).to(torch.bfloat16)], dim=1)
    x0 = rec["cross.0"]["in"][0]
    assert x0.shape[1] == m.in_dim == feats.shape[1] + m.pad
    assert torch.equal(_bits(x0), _bits(torch.nn.functional.pad(feats, (0, m.pad))))
    assert torch.equal(_bits(rec["deep"]["in"][0]), _bits(x0))
    xl = x0
    for l, c in enumerate(m.cross):
        r = rec[f"cross.{l}"]
        assert torch.equal(_bits(r["in"][0]), _bits(x0))
        assert torch.equal(_bits(r["in"][1]), _bits(xl))
        proj = rec[f"cross.{l}." + ("w" if c.w is not None else "u")]
        if c.w is None:  # u reads v's output
            assert torch.equal(_bits(proj["in"][0]), _bits(rec[f"cross.{l}.v"]["out"]))
            assert torch.equal(_bits(rec[f"cross.{l}.v"]["in"][0]), _bits(xl))
        T.worst_ratio(r["out"], *T.cross_mix_model(x0, proj["out"], xl),
                      "cross mix", log)
        T.worst_ratio(proj["gout"], *T.cross_dproj_model(r["gout"], x0),
                      "cross dproj", log)
        xl = r["out"]
    head_in = rec["head"]["in"][0]
    assert torch.equal(_bits(head_in),
                       _bits(torch.cat([xl, rec["deep"]["out"]], dim=1)))


def _merge(dst, src):
    for k, v in src.items():
        kind = " ".join(k.split(" ")[1:]) if "." in k.split(" ")[0] else k
        dst[kind] = max(dst.get(kind, 0.0), v)


STAGE_CASES = [n for n in T.CASES]


@pytest.mark.parametrize("name", STAGE_CASES)
def test_stage_chain(name):
    kind = T.CASES[name][0]
    lay, ch = _layered(name), _chain(name)
    _assert_paths(name, lay, True)
    _assert_paths(name, ch, False)
    models, log = _layer_models(name)
    layers_l, layers_c = _fused_layers(lay["model"]), _fused_layers(ch["model"])
    _check_param_grads(models, layers_l, _module_grads, log, "per-layer")
    _check_param_grads(models, layers_c, _module_grads, log, "chain")
    # the chained run reproduces the per-layer run's forward and dx bits
    assert torch.equal(_bits(ch["logits"]), _bits(lay["logits"]))
    assert torch.equal(_bits(ch["dense"].grad), _bits(lay["dense"].grad))
    ge_c = ch["emb"].grad if torch.is_tensor(ch["emb"]) else \
        torch.cat([e.grad for e in ch["emb"]])
    ge_l = lay["emb"].grad if torch.is_tensor(lay["emb"]) else \
        torch.cat([e.grad for e in lay["emb"]])
    assert torch.equal(_bits(ge_c), _bits(ge_l))
    for c in _containers(ch["model"], kind):
        for key in ("out", "gout"):
            assert torch.equal(_bits(ch["tape"].rec[c][key]),
                               _bits(lay["tape"].rec[c][key])), (c, key)
        assert torch.equal(_bits(ch["tape"].rec[c]["gin"][0]),
                           _bits(lay["tape"].rec[c]["gin"][0])), c
    for run in (lay, ch):
        if kind == "dlrm":
            _check_dlrm_glue(run, log)
        else:
            _check_dcn_glue(run, log)
    summary = {}
    _merge(summary, log)
    print(f"{name} worst err/bound per stage:",
          {k: float(f"{v:.3g}") for k, v in sorted(summary.items())})


def test_dlrm_prepadded_top_input_widths():
    """dx of the pre-padded top input is k + pad wide inside the chain; the
    parameter gradients come back in the stored widths."""
    for name in ("dlrm-small", "dlrm-bench"):
        ch = _chain(name)
        m = ch["model"]
        k = m.top.layers[0].weight.shape[1]
        assert k % 128 != 0
        gin = ch["tape"].rec["top"]["gin"][0]
        assert gin.shape[1] == T._kp(k) and (gin[:, k:] == 0).all()
        for _, mod in _fused_layers(m):
            assert mod.weight.grad.shape == mod.weight.shape
            assert mod.weight.grad.dtype == mod.weight.dtype
    assert _chain("dlrm-bench")["model"].top.layers[0].weight.shape == (1024, 479)


def test_sideband_slots():
    """dlrm-small with a side-band slot on every fused weight and bias: the
    slots meet the same bounds, dx and dbase keep their bits, a second
    backward adds."""
    ref = _chain("dlrm-small")
    models, _ = _layer_models("dlrm-small")
    log = {}
    for backwards in (1, 2):
        run = _run_fused("dlrm-small", side=True, backwards=backwards)
        layers = _fused_layers(run["model"])
        assert len(run["slots"]) == len(layers) == 4
        for _, mod in layers:
            assert mod.weight.grad is None and mod.bias.grad is None
        _check_param_grads(models, layers, lambda n, mod: run["slots"][n], log,
                           f"slot x{backwards}", f32=True, scale=backwards)
        assert torch.equal(_bits(run["logits"]), _bits(ref["logits"]))
        if backwards == 1:
            assert torch.equal(_bits(run["dense"].grad), _bits(ref["dense"].grad))
            assert torch.equal(_bits(run["emb"].grad), _bits(ref["emb"].grad))
    print("sideband worst err/bound:", max(log.values()))


# -------------------------------------------------------- b. whole-tower net
def _eager_run(name):
    """The eager bf16 tower with the fused tower's parameter bits."""
    kind, _, _, _, _ = T.CASES[name]
    mf = _chain(name)["model"]
    me = T.make_model(name, False, _dev()).bfloat16()
    if kind == "dlrm":
        pe, pf = list(me.parameters()), list(mf.parameters())
        assert len(pe) == len(pf)
        with torch.no_grad():
            for a, b in zip(pe, pf):
                a.copy_(b)
    else:
        T.copy_dcn_fused_to_eager(mf, me)
    dense, emb, y = T.make_inputs(name, _dev())
    logits = me(dense, emb)
    torch.nn.functional.binary_cross_entropy_with_logits(logits.float(), y).backward()
    params_of = T.dlrm_params if kind == "dlrm" else T.dcn_params
    return me, T.module_result(me, params_of, logits, dense, emb)


def test_eager_bf16_dlrm_takes_the_packed_base():
    """The eager tower on the packed f16 base runs the packed interaction
    too; only a fused top may be handed the pre-padded input (an nn.Linear
    top rejected the 128-wide input of this shape before the pad was tied
    to `fused`)."""
    me = T.make_model("dlrm-small", False, _dev())
    dense, base, _ = T.make_inputs("dlrm-small", _dev())
    logits = me(dense, base)
    assert logits.shape == (200,)
    assert "_InteractPackedFnBackward" in T.grad_fn_names(logits)


@pytest.mark.parametrize("name", STAGE_CASES)
def test_whole_tower_against_twin(name):
    kind = T.CASES[name][0]
    ch = _chain(name)
    mf = ch["model"]
    params_of, twin_fn = (T.dlrm_params, T.dlrm_f64) if kind == "dlrm" else \
        (T.dcn_params, T.dcn_f64)
    twin = twin_fn(params_of(mf), ch["dense"], ch["emb"], ch["y"])
    got = T.module_result(mf, params_of, ch["logits"], ch["dense"], ch["emb"])
    e_fused = T.rel_errs(got, twin)
    me, got_e = _eager_run(name)
    ref_e = T.flat(twin) if kind == "dlrm" else T.dcn_unpad(twin, me.in_dim, mf.in_dim)
    flat_e = T.flat(got_e)
    bad = []
    for k, ef in e_fused.items():
        ee = T.rel_err(flat_e[k], ref_e[k])
        print(f"{name} {k}: e_fused {ef:.3e} e_eager {ee:.3e} "
              f"ratio to gate {ef / T.gate(ee):.3g}")
        if not ef <= T.gate(ee):
            bad.append((k, ef, ee))
    assert len(e_fused) == len(list(mf.parameters())) + 3
    assert not bad, bad
    loss = torch.nn.functional.binary_cross_entropy_with_logits(
        ch["logits"].double(), ch["y"].double())
    assert abs(loss.item() - twin["loss"].item()) <= \
        T.gate(0.0) * max(abs(twin["loss"].item()), 1.0)


# ---------------------------------------------------------- c. exact structure
def _pad_grads(m):
    """Every gradient block that multiplies a pad feature."""
    in_e, in_p = m.in_dim - m.pad, m.in_dim
    out = {}
    for l, c in enumerate(m.cross):
        if c.w is not None:
            out[f"cross.{l}.w cols"] = c.w.weight.grad[:, in_e:]
            out[f"cross.{l}.w rows"] = c.w.weight.grad[in_e:]
            out[f"cross.{l}.w bias"] = c.w.bias.grad[in_e:]
        else:
            out[f"cross.{l}.v cols"] = c.v.weight.grad[:, in_e:]
            out[f"cross.{l}.u rows"] = c.u.weight.grad[in_e:]
            out[f"cross.{l}.u bias"] = c.u.bias.grad[in_e:]
    out["deep.0 cols"] = m.deep.layers[0].weight.grad[:, in_e:]
    out["head pad block"] = m.head.weight.grad[:, in_e:in_p]
    return out


@pytest.mark.parametrize("name", ["dcn-lowrank", "dcn-full"])
def test_dcn_pad_gradients_are_exactly_zero(name):
    from persia_amd.ops.dense import fused_bce_with_logits

    run = _run_fused(name)
    m = run["model"]
    assert m.pad == 19
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for step in range(2):
        blocks = _pad_grads(m)
        assert len(blocks) == 3 * len(m.cross) + 2
        for k, g in blocks.items():
            assert g.numel() > 0 and (g == 0).all(), (step, k)
        for c in m.cross:
            if c.w is None:
                assert c.v.bias.grad is None and (c.v.bias == 0).all()
                assert not isinstance(c.v.bias, torch.nn.Parameter)
        if step == 0:
            torch.optim.SGD(m.parameters(), lr=0.1).step()
            moved = [k for k, v in m.state_dict().items()
                     if not torch.equal(v, before[k])]
            assert len(moved) == len(list(m.parameters())), moved
            for p in m.parameters():
                p.grad = None
            fused_bce_with_logits(m(run["dense"], run["emb"]), run["y"]).backward()


@pytest.mark.parametrize("name", ["dcn-lowrank", "dcn-full", "dcn-nopad"])
def test_dcn_packed_base_equals_list_of_slots(name):
    a, b = _chain(name), _run_fused(name, as_list=True)
    B = a["dense"].shape[0]
    assert torch.equal(_bits(a["logits"]), _bits(b["logits"]))
    assert torch.equal(_bits(a["dense"].grad), _bits(b["dense"].grad))
    for s, e in enumerate(b["emb"]):
        assert torch.equal(_bits(a["emb"].grad[s * B:(s + 1) * B]), _bits(e.grad))
    # The dx path carries no atomics, so everything above is bit for bit.
    # The weight and bias gradients are split-M atomic sums (M = 200 on a
    # 128x128 weight: 4 parts) whose order the hardware picks: identical
    # addends, not identical bits.  They are held to the stage models of the
    # packed run, whose stage inputs the list run shares bit for bit.
    for c in _containers(a["model"], "dcn"):
        for key in ("out", "gout"):
            assert torch.equal(_bits(a["tape"].rec[c][key]),
                               _bits(b["tape"].rec[c][key])), (c, key)
    models, _ = _layer_models(name)
    _check_param_grads(models, _fused_layers(b["model"]), _module_grads, {}, "list")
    for k in ("weight", "bias"):  # the head: one torch GEMM, no atomics
        assert torch.equal(_bits(getattr(a["model"].head, k).grad),
                           _bits(getattr(b["model"].head, k).grad))


# --------------------------------------------------------- d. negative control
def test_swapped_slots_violate_the_interaction_bound():
    run = _run_fused("dlrm-small", swap=True)
    good = _chain("dlrm-small")
    # the stage model of the UNSWAPPED base
    with pytest.raises(AssertionError, match="interaction fwd"):
        _check_dlrm_glue(run, {}, emb_bsd=_emb_bsd(good), only_inter=True)
    _check_dlrm_glue(run, {}, only_inter=True)  # and holds for its own base


# ----------------------------------------------------------------------- e. BCE
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("n", T.BCE_SIZES)
def test_bce_exact(n, soft):
    from persia_amd.ops.dense import fused_bce_with_logits

    C = _native()
    z32, y = T.bce_case(n, soft, _dev())
    z_bf = z32.to(torch.bfloat16)
    if n >= len(T.BCE_PLANTED):
        for v in T.BCE_PLANTED:
            assert (z_bf == v).any(), v
    zf = z_bf.float()
    n_blocks = (n + 255) // 256
    for scale in T.BCE_SCALES:
        z = z_bf.clone().requires_grad_(True)
        loss = fused_bce_with_logits(z, y)
        (loss * scale).backward()
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert z.grad.dtype == torch.bfloat16
        loss2, sig = C.bce_fwd(zf, y)
        g = torch.tensor([scale], device=_dev())
        dz = C.bce_bwd(sig, y, g)
        mdl = T.bce_model(zf, y, g, sig, T.EXP_ULPS, T.LOG_ULPS)
        T.worst_ratio(loss, *mdl["loss"], f"bce loss n={n}")
        T.worst_ratio(sig, *mdl["sig"], f"bce sig n={n}")
        T.worst_ratio(dz, *mdl["dz"], f"bce dz n={n} scale={scale}")
        # the bf16 dz is the f32 kernel result, rounded once
        assert torch.equal(_bits(z.grad), _bits(dz.to(torch.bfloat16)))
        for t in (loss, sig, dz, z.grad):
            assert torch.isfinite(t).all()
        # a fresh accumulator each call: up to two blocks any atomic order
        # gives the same bits; beyond, the calls differ by at most the
        # reordering of n_blocks addends
        if n_blocks <= 2:
            assert torch.equal(_bits(loss.view(1)), _bits(loss2.view(1)))
        else:
            tot = (mdl["loss"][0].abs() + mdl["loss"][1]).item()
            assert abs(loss.item() - loss2.item()) <= n_blocks * T.U24 * tot


def bce_sweep():
    """-> (z, y, sig, terms) of the kernel on the dense sweep."""
    C = _native()
    z = torch.linspace(-100, 100, 400001, device=_dev(), dtype=torch.float64).float()
    y = torch.zeros_like(z)
    _, sig = C.bce_fwd(z, y)
    zt = torch.linspace(-100, 100, 4001, device=_dev(), dtype=torch.float64).float()
    gen = torch.Generator().manual_seed(3)
    yt = torch.rand(4001, generator=gen).to(_dev())
    terms = torch.stack([C.bce_fwd(zt[i:i + 1], yt[i:i + 1])[0]
                         for i in range(zt.numel())])
    return z, y, sig, zt, yt, terms


def test_bce_intrinsics_within_the_measured_constants():
    """The sweep the constants were measured on: the kernel needs no more
    than half of EXP_ULPS / LOG_ULPS."""
    z, y, sig, zt, yt, terms = bce_sweep()
    exp_need = T.bce_exp_ulps_needed(z, sig)
    s64, E, t64, Et = T.bce_terms_bound(zt.double(), yt.double(),
                                        T.EXP_ULPS, T.LOG_ULPS)
    print(f"bce sweep: exp ulps needed {exp_need:.3f} (constant {T.EXP_ULPS})")
    assert exp_need <= T.EXP_ULPS / 2 + 1e-9
    T.worst_ratio(terms, t64, Et, "bce term sweep")
    assert torch.isfinite(sig).all() and torch.isfinite(terms).all()
