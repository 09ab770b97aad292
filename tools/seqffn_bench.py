"""The tail of a transformer block over a raw slot: the eager reference and an
f16 torch composition against the HIP kernels (csrc/seqffn.hip), alternating
in one process.

Shapes: the raw slot of tools/seqsa_bench.py -- per-GPU batch 4096, dim 64,
ffn 256, ``sample_fixed_size`` 50 with lengths uniform in 0..80 clipped to the
slot's size -- and a short one (``sample_fixed_size`` 20, lengths 0..32).  A
step is forward plus backward of ``seq_ffn`` from a fixed f16 gradient, with
gradients for ``x``, ``a`` and all ten parameters; ``a`` is the output of
``seq_self_attn`` (2 heads) on ``x``, computed once.  "eager" is what
``PA_SEQ_FFN=0`` runs (ops/reference.py on the GPU), "native" the kernels.
"f16" is what a user would write without either: slice the rows, f16
``F.linear`` and ``F.layer_norm`` on all of them -- for orientation: it
rounds elsewhere, runs the padding rows and leaves their outputs in place.

Each path first makes a warm-up pass, then ``--steps`` steps are timed with
device events, ending in a synchronise.  The paths alternate, and the whole
thing repeats ``--reps`` times for the spread.  Reported per shape and path:
the median ms/step and its min/max over the repetitions, and the largest
difference between the eager and native results.  One JSON line per shape.

Run: python tools/seqffn_bench.py [--steps 100] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from persia_amd.ops import seqffn
from persia_amd.ops.seqsa import seq_self_attn
from seqattn_bench import make_inputs
from seqsa_bench import timed

SHAPES = [(4096, 50, 64, 256, 2, 80), (4096, 20, 64, 256, 2, 32)]  # B L D F heads max_len
PARAMS = ("Wo", "bo", "g1", "be1", "W1", "b1", "W2", "b2", "g2", "be2")
NAMES = ("out", "dx", "da") + tuple("d" + n for n in PARAMS)


def step(use_native, leaves, g):
    seqffn._ENABLED = use_native  # what PA_SEQ_FFN sets at import
    for t in leaves:
        t.grad = None
    out = seqffn.seq_ffn(*leaves)
    out.backward(g)
    return out


def results(use_native, leaves, g):
    out = step(use_native, leaves, g)
    return [out.detach().float()] + [t.grad.detach().float() for t in leaves]


def f16_step(x, a, p, g):
    for t in (x, a, *p):
        t.grad = None
    Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2 = p
    D = x.shape[-1]
    u = F.layer_norm(x + F.linear(a, Wo, bo), (D,), g1, be1)
    y = F.layer_norm(u + F.linear(F.relu(F.linear(u, W1, b1)), W2, b2), (D,), g2, be2)
    y.backward(g)


def bench(shape, steps, reps, device):
    B, L, D, Fh, heads, max_len = shape
    _, x, _, cells = make_inputs(B, L, D, max_len, device)
    gen = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    Wqkv, bqkv = (r(3 * D, D) * D ** -0.5).to(device), (r(3 * D) * 0.1).to(device)
    a = seq_self_attn(x, Wqkv, bqkv, heads).detach()
    par = [r(D, D) * D ** -0.5, r(D) * 0.1, 1 + r(D) * 0.1, r(D) * 0.1,
           r(Fh, D) * D ** -0.5, r(Fh) * 0.1, r(D, Fh) * Fh ** -0.5, r(D) * 0.1,
           1 + r(D) * 0.1, r(D) * 0.1]
    g = (r(B, L, D + 1) * 0.5).half().to(device)
    leaves = [t.to(device).requires_grad_(True) for t in (x, a, *par)]
    x16, a16 = (t.detach()[..., :D].contiguous().requires_grad_(True) for t in (x, a))
    p16 = [t.detach().half().to(device).requires_grad_(True) for t in par]
    g16 = g[..., :D].contiguous()
    paths = {"eager": lambda: step(False, leaves, g),
             "f16": lambda: f16_step(x16, a16, p16, g16),
             "native": lambda: step(True, leaves, g)}
    taken = {n: type(step(n == "native", leaves, g).grad_fn).__name__
             for n in ("eager", "native")}
    assert taken["native"] == "SeqFfnFnBackward" and \
        taken["eager"] != taken["native"], taken
    for fn in paths.values():  # warm-up pass
        timed(fn, 3)
    diffs = [float((p - q).abs().max()) for p, q in
             zip(results(False, leaves, g), results(True, leaves, g))]
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            ms[name].append(timed(fn, steps))
    out = {"shape": dict(batch=B, sfs=L, max_len=max_len, dim=D, ffn=Fh,
                         valid_cells=cells, steps=steps, reps=reps)}
    for name in paths:
        out[name] = dict(
            ms_per_step_median=round(statistics.median(ms[name]), 4),
            ms_per_step_min=round(min(ms[name]), 4),
            ms_per_step_max=round(max(ms[name]), 4),
        )
    out["max_abs_diff"] = dict(zip(NAMES, diffs))
    out["speedup_median"] = {
        k: round(out[k]["ms_per_step_median"] / out["native"]["ms_per_step_median"], 3)
        for k in ("eager", "f16")}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    for shape in SHAPES:
        bench(shape, args.steps, args.reps, device)


if __name__ == "__main__":
    main()
