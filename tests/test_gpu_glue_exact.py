"""The DLRM glue kernels against what they replace (cases, references and
bounds: tests/test_glue_cases_cpu.py).

* interact_fwd_top / interact_bwd_top: bit-equal to cat([x,
  interact_fwd_packed, zeros]) and to interact_bwd_packed on the sliced pair
  block plus autograd's bf16 sum for dx; pad columns of g are never read; a
  pair block shifted by one column is told apart.
* head_fwd / head_bwd: logit, dw, db inside their bounds on the input bits,
  dh bit-equal, dw / db equal between two calls (fixed-order reduction).
* pad_k: bit-equal to F.pad.
* dlrm-small: PA_INTERACT_TOP=0 against the default bit for bit; the head
  stage inside its bounds with PA_NATIVE_HEAD=0 and with the default; forward
  + backward captured in a graph and replayed against the eager run.

One thing the issue states differently, for a reason in the kernels (the one
tests/test_gpu_tower_exact.py documents): the fused layers' weight and bias
gradients are split-M f32 atomic sums whose order the hardware picks, so two
runs of the same code need not agree in their bits.  Under PA_INTERACT_TOP
on / off and under graph replay they are therefore held to one bf16 rounding
(relative L2 difference <= 2^-8), while everything with a fixed order --
logits, dense.grad, emb.grad, the bottom output and its summed gradient, the
top input's gradient, the head's dw / db -- is compared bit for bit; with
every stage's inputs bit-equal, the atomic sums add identical addends.

Measured on an MI355X: all comparisons above bit-equal; worst err/bound head
logit 0.993, dw 0.896, db 0.300 (kernel cases), 0.938 / 0.800 / 0 in the model.
"""
import pytest
import torch

import test_glue_cases_cpu as G
import test_tower_cases_cpu as T
from test_gpu_dense_exact import _bits

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _native():
    from persia_amd.ops import native

    return native()


# --------------------------------------------------------------- interaction
def _check_top(C, x, base, g, pad, g_ref=None):
    """interact_*_top on (x, base, g) against the composition on g_ref."""
    B, D = x.shape
    P = G.n_pairs(base.shape[0] // B)
    g_ref = g if g_ref is None else g_ref
    out = C.interact_fwd_top(x, base, pad)
    assert out.shape == (B, D + P + pad) and out.dtype == torch.bfloat16
    want = G.top_fwd_composition(x, C.interact_fwd_packed(x, base), pad)
    assert torch.equal(_bits(out), _bits(want)), "top input"
    dx, dbase = C.interact_bwd_top(g, x, base)
    dx0, dbase0 = C.interact_bwd_packed(g_ref[:, D:D + P].contiguous(), x, base)
    assert dbase.dtype == torch.float16 and dbase.shape == base.shape
    assert torch.equal(_bits(dbase), _bits(dbase0)), "dbase"
    assert torch.equal(_bits(dx), _bits(G.top_bwd_composition(g_ref, dx0, D))), "dx"
    return dx, dbase


@pytest.mark.parametrize("S,D", G.INTERACT_SD)
def test_interact_top_exact(S, D):
    C = _native()
    assert C.interact_packed_feasible(S + 1, D)
    P = G.n_pairs(S)
    for B in G.INTERACT_B:
        for pad in G.pads_of(S, D):
            x, base, g = G.interact_case(B, S, D, pad, _dev())
            dx, dbase = _check_top(C, x, base, g, pad)
            if pad:  # the pad columns are never read
                g_nan = g.clone()
                g_nan[:, D + P:] = float("nan")
                dx2, dbase2 = C.interact_bwd_top(g_nan, x, base)
                assert torch.equal(_bits(dx2), _bits(dx))
                assert torch.equal(_bits(dbase2), _bits(dbase))
                assert not dx2.isnan().any() and not dbase2.isnan().any()
            if P > 1:  # negative control
                with pytest.raises(AssertionError, match="dbase"):
                    _check_top(C, x, base, g, pad, g_ref=G.shift_pairs(g, D, P))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- head
@pytest.mark.parametrize("K", G.HEAD_K)
@pytest.mark.parametrize("B", G.HEAD_B)
def test_head_exact(B, K):
    C = _native()
    h, w, b, dz = G.head_case(B, K, _dev())
    mdl = G.head_model(h, w, b, dz)
    logit = C.head_fwd(h, w, b)
    assert logit.shape == (B, 1) and logit.dtype == torch.bfloat16
    G.within(logit, *mdl["logit"], f"head logit {B}x{K}")
    dh, dw, db = C.head_bwd(dz, h, w)
    assert dh.shape == h.shape and dw.shape == w.shape and db.shape == b.shape
    assert torch.equal(_bits(dh), _bits(G.head_dh_reference(dz, w)))
    G.within(dw, *mdl["dw"], f"head dw {B}x{K}")
    G.within(db.view(1), *mdl["db"], f"head db {B}x{K}")
    _, dw2, db2 = C.head_bwd(dz, h, w)
    assert torch.equal(_bits(dw2), _bits(dw)) and torch.equal(_bits(db2), _bits(db))


# --------------------------------------------------------------------- pad_k
@pytest.mark.parametrize("shape", G.PAD_K_SHAPES)
def test_pad_k_exact(shape):
    from persia_amd.ops.dense import _pad32

    C = _native()
    w = G.pad_k_case(*shape, _dev())
    want = G.pad_k_reference(w)
    for got in (C.pad_k(w, 128), _pad32(w, 1)):
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    if shape[1] % 128 == 0:
        assert C.pad_k(w, 128).data_ptr() == w.data_ptr()


# --------------------------------------------------------------- model level
NAME = "dlrm-small"


def _run(monkeypatch, **env):
    from persia_amd.ops.dense import fused_bce_with_logits

    for k in ("PA_INTERACT_TOP", "PA_NATIVE_HEAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = T.make_model(NAME, True, _dev())
    dense, emb, y = T.make_inputs(NAME, _dev())
    tape = T.Tape(model, ("bottom", "top"))
    logits = model(dense, emb)
    names = T.grad_fn_names(logits)
    fused_bce_with_logits(logits, y).backward()
    tape.close()
    torch.cuda.synchronize()
    return dict(model=model, tape=tape, logits=logits.detach(), dense=dense,
                emb=emb, names=names)


def test_interact_top_knob_is_bit_equal(monkeypatch):
    a = _run(monkeypatch)
    b = _run(monkeypatch, PA_INTERACT_TOP="0")
    assert "CatBackward0" in b["names"] and "CatBackward0" not in a["names"]
    assert "_InteractPackedFnBackward" in a["names"]
    for k in ("logits", "dense", "emb"):
        ta, tb = (r[k] if k == "logits" else r[k].grad for r in (a, b))
        assert torch.equal(_bits(ta), _bits(tb)), k
    # the dx path carries no atomics, so every stage received the same bits;
    # the fused layers' dw / db are split-M atomic sums (order not fixed), so
    # they are compared inside one bf16 rounding, the head's bit for bit
    pa, pb = dict(a["model"].named_parameters()), dict(b["model"].named_parameters())
    for n in pa:
        if n.startswith("top.layers.2."):
            assert torch.equal(_bits(pa[n].grad), _bits(pb[n].grad)), n
        else:
            assert T.rel_err(pa[n].grad, pb[n].grad) <= T.GATE_FLOOR, n
    for c in ("bottom", "top"):
        for key in ("out", "gout"):
            assert torch.equal(_bits(a["tape"].rec[c][key]),
                               _bits(b["tape"].rec[c][key])), (c, key)


@pytest.mark.parametrize("native_head", ["1", "0"])
def test_head_stage_bounds_in_the_model(monkeypatch, native_head):
    run = _run(monkeypatch, PA_NATIVE_HEAD=native_head)
    assert ("_HeadFnBackward" in run["names"]) == (native_head == "1")
    head = run["model"].top.layers[-1]
    rec = run["tape"].rec["top.layers.2"]
    h, out, dz, dh = rec["in"][0], rec["out"], rec["gout"], rec["gin"][0]
    mdl = G.head_model(h, head.weight, head.bias, dz)
    G.within(out, *mdl["logit"], "model head logit")
    assert torch.equal(_bits(run["logits"]), _bits(out.squeeze(1)))
    assert torch.equal(_bits(dh), _bits(G.head_dh_reference(dz, head.weight.detach())))
    G.within(head.weight.grad, *mdl["dw"], "model head dw")
    G.within(head.bias.grad, *mdl["db"], "model head db")


def test_graph_capture_and_replays_match_eager(monkeypatch):
    from persia_amd.ops.dense import fused_bce_with_logits

    for k in ("PA_INTERACT_TOP", "PA_NATIVE_HEAD"):
        monkeypatch.delenv(k, raising=False)
    model = T.make_model(NAME, True, _dev())
    dense, emb, y = T.make_inputs(NAME, _dev())
    leaves = [dense, emb] + list(model.parameters())

    def step():
        for t in leaves:
            t.grad = None
        logits = model(dense, emb)
        fused_bce_with_logits(logits, y).backward()
        return logits.detach()  # no autograd graph kept alive across steps

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            logits = step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = [logits.detach().clone()] + [t.grad.clone() for t in leaves]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits = step()
    n_head = 2  # the head's weight and bias: fixed-order sums
    for _ in range(3):
        for t in leaves:
            t.grad.fill_(7.0)  # a replay has to overwrite every gradient
        graph.replay()
        torch.cuda.synchronize()
        got = [logits.detach()] + [t.grad for t in leaves]
        exact = (0, 1, 2, len(got) - 2, len(got) - 1)  # no atomics on these
        for i, (a, b) in enumerate(zip(got, eager)):
            if i in exact:
                assert torch.equal(_bits(a), _bits(b)), i
            else:  # split-M atomic sums: one bf16 rounding apart at most
                assert T.rel_err(a, b) <= T.GATE_FLOOR, i
    assert n_head == sum(1 for _ in model.top.layers[-1].parameters())
