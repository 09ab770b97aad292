"""Self-attention over a raw slot: the eager reference and an f16 SDPA
composition against the HIP kernels (csrc/seqsa.hip), alternating in one
process.

Shapes: the raw slot of tools/raw_bench.py -- per-GPU batch 4096, dim 64, 2
heads, ``sample_fixed_size`` 50 with lengths uniform in 0..80 clipped to the
slot's size -- and a short one (``sample_fixed_size`` 20, lengths 0..32).  A
step is forward plus backward of ``seq_self_attn`` with a residual, from a
fixed f16 gradient, with gradients for the sequence, ``Wqkv`` and ``bqkv``.
"eager" is what ``PA_SEQ_SELF_ATTN=0`` runs (ops/reference.py on the GPU),
"native" the kernels.  "sdpa" is what a user would write without either: slice
the rows, an f16 ``linear`` to ``[B, L, 3D]``, a boolean ``[B, 1, L, L]`` mask
and ``F.scaled_dot_product_attention`` -- for orientation: it rounds
elsewhere and leaves the invalid rows' outputs in place.

Each path first makes a warm-up pass, then ``--steps`` steps are timed with
device events, ending in a synchronise.  The paths alternate, and the whole
thing repeats ``--reps`` times for the spread.  Reported per shape and path:
the median ms/step and its min/max over the repetitions, and the largest
difference between the eager and native results.  One JSON line per shape.

Run: python tools/seqsa_bench.py [--steps 100] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from persia_amd.ops import seqsa
from seqattn_bench import make_inputs

SHAPES = [(4096, 50, 64, 2, 80), (4096, 20, 64, 2, 32)]  # B, L, D, heads, max_len
NAMES = ("out", "dseq", "dWqkv", "dbqkv")


def step(use_native, leaves, heads, g):
    seqsa._ENABLED = use_native  # what PA_SEQ_SELF_ATTN sets at import
    for t in leaves:
        t.grad = None
    out = seqsa.seq_self_attn(*leaves, heads, residual=True)
    out.backward(g)
    return out


def results(use_native, leaves, heads, g):
    out = step(use_native, leaves, heads, g)
    return [out.detach().float()] + [t.grad.detach().float() for t in leaves]


def sdpa_step(x, valid, W16, b16, heads, g):
    x.grad = W16.grad = b16.grad = None
    B, L, D = x.shape
    q, k, v = (F.linear(x, W16, b16).reshape(B, L, 3, heads, D // heads)
               .permute(2, 0, 3, 1, 4))
    allowed = valid[:, None, None, :] | torch.eye(L, dtype=torch.bool,
                                                  device=x.device)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=allowed)
    (o.transpose(1, 2).reshape(B, L, D) + x).backward(g)


def timed(fn, steps):
    """-> ms/step by device events."""
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps


def bench(shape, steps, reps, device):
    B, L, D, heads, max_len = shape
    _, seq, _, cells = make_inputs(B, L, D, max_len, device)
    gen = torch.Generator().manual_seed(2)
    W = (torch.randn(3 * D, D, generator=gen) * D ** -0.5).to(device)
    b = (torch.randn(3 * D, generator=gen) * 0.1).to(device)
    g = (torch.randn(B, L, D + 1, generator=gen) * 0.5).half().to(device)
    leaves = [t.requires_grad_(True) for t in (seq, W, b)]
    x = seq.detach()[..., :D].contiguous().requires_grad_(True)
    valid = seq.detach()[..., D] != 0
    W16, b16 = (t.detach().half().requires_grad_(True) for t in (W, b))
    g16 = g[..., :D].contiguous()
    paths = {"eager": lambda: step(False, leaves, heads, g),
             "sdpa": lambda: sdpa_step(x, valid, W16, b16, heads, g16),
             "native": lambda: step(True, leaves, heads, g)}
    taken = {n: type(step(n == "native", leaves, heads, g).grad_fn).__name__
             for n in ("eager", "native")}
    assert taken["native"] == "SeqSelfAttnFnBackward" and \
        taken["eager"] != taken["native"], taken
    for fn in paths.values():  # warm-up pass
        timed(fn, 3)
    diffs = [float((a - c).abs().max()) for a, c in
             zip(results(False, leaves, heads, g), results(True, leaves, heads, g))]
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            ms[name].append(timed(fn, steps))
    out = {"shape": dict(batch=B, sfs=L, max_len=max_len, dim=D, heads=heads,
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
        for k in ("eager", "sdpa")}
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
