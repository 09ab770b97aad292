"""Self-attention over a long raw slot: the eager reference and an f16 SDPA
composition against the streamed-key HIP kernels (csrc/seqsal.hip),
alternating in one process.

Shapes: per-GPU batch 4096, dim 64, 2 heads, ``sample_fixed_size`` 200 (the
length tools/actunit_bench.py and tools/seqgru_bench.py run) and 100, lengths
uniform in 0..1.6 L clipped to L.  A step is forward plus backward of
``seq_self_attn_long`` with a residual, from a fixed f16 gradient, with
gradients for the sequence, ``Wqkv`` and ``bqkv``.  "eager" is what
``PA_SEQ_SELF_ATTN_LONG=0`` runs (ops/reference.py on the GPU, what the models
ran at these lengths before the kernels), "native" the kernels, "sdpa" the
composition of tools/seqsa_bench.py, for orientation.

Each path first makes a warm-up pass, then ``--steps`` steps are timed with
device events, ending in a synchronise.  The paths alternate, and the whole
thing repeats ``--reps`` times for the spread.  Reported per shape and path:
the median ms/step and its min/max over the repetitions, and the largest
difference between the eager and native results.  One JSON line per shape.

Run: python tools/seqsal_bench.py [--steps 100] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from persia_amd.ops import seqsal
from seqattn_bench import make_inputs
from seqsa_bench import NAMES, sdpa_step, timed

SHAPES = [(4096, 200, 64, 2, 320), (4096, 100, 64, 2, 160)]  # B, L, D, heads, max_len


def step(use_native, leaves, heads, g):
    seqsal._ENABLED = use_native  # what PA_SEQ_SELF_ATTN_LONG sets at import
    for t in leaves:
        t.grad = None
    out = seqsal.seq_self_attn_long(*leaves, heads, residual=True)
    out.backward(g)
    return out


def results(use_native, leaves, heads, g):
    out = step(use_native, leaves, heads, g)
    return [out.detach().float()] + [t.grad.detach().float() for t in leaves]


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
    assert taken["native"] == "SeqSelfAttnLongFnBackward" and \
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
    out["native_max_below_eager_min"] = (
        out["native"]["ms_per_step_max"] < out["eager"]["ms_per_step_min"])
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
