"""GRU / AUGRU sequence benchmark: the eager torch loop against the HIP
kernels (csrc/seqgru.hip), alternating in one process.

Shapes: the raw slot of tools/raw_bench.py -- per-GPU batch 4096,
``sample_fixed_size`` 50, dim 64, lengths uniform in 0..80 clipped to the
slot's size -- with 64 hidden units, and once a long one (``sample_fixed_size``
200, lengths 0..320).  A step is forward plus backward of ``seq_gru`` with an
attention weight per row (AUGRU), from fixed f16 gradients of ``states`` and
``last``, with gradients for the sequence, the four parameters and ``att``.
"eager" is what ``PA_SEQ_GRU=0`` runs (ops/reference.py on the GPU, a Python
loop over the steps), "native" the kernels.  "nn_gru" is ``torch.nn.GRU`` in
f16 on the same rows, forward plus backward -- for orientation only: it
computes another function (every row counts, no ``att``).

Each path first makes a warm-up pass, then ``--steps`` steps are timed with
device events, ending in a synchronise.  The paths alternate, and the whole
thing repeats ``--reps`` times for the spread.  Reported per shape and path:
the median ms/step and its min/max over the repetitions, and the largest
difference between the eager and native results.  One JSON line per shape.

Run: python tools/seqgru_bench.py [--steps 100] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from persia_amd.ops import seqgru
from seqattn_bench import make_inputs

SHAPES = [(4096, 50, 64, 64, 80), (4096, 200, 64, 64, 320)]  # B, L, D, H, max_len


def make_params(D, H, device):
    gen = torch.Generator().manual_seed(1)
    Wx = torch.randn(3 * H, D, generator=gen) * (0.5 * D ** -0.5)
    Wh = torch.randn(3 * H, H, generator=gen) * (0.5 * H ** -0.5)
    bx, bh = (torch.randn(3 * H, generator=gen) * 0.1 for _ in range(2))
    return [p.to(device).requires_grad_(True) for p in (Wx, Wh, bx, bh)]


def step(use_native, leaves, grads):
    seqgru._ENABLED = use_native  # what PA_SEQ_GRU sets at import
    for t in leaves:
        t.grad = None
    outs = seqgru.seq_gru(*leaves)
    torch.autograd.backward(outs, grads)
    return outs


def results(use_native, leaves, grads):
    outs = step(use_native, leaves, grads)
    return [o.detach().float() for o in outs] + [t.grad.detach().float() for t in leaves]


def gru_step(gru, x, grads):
    x.grad = None
    gru.zero_grad(set_to_none=True)
    states, hn = gru(x)
    torch.autograd.backward([states, hn[0]], grads)


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
    B, L, D, H, max_len = shape
    _, seq, _, cells = make_inputs(B, L, D, max_len, device)
    gen = torch.Generator().manual_seed(2)
    att = (torch.rand(B, L, generator=gen) * 0.98 + 0.01).to(device)
    grads = [(torch.randn(*s, generator=gen) * 0.5).half().to(device)
             for s in ((B, L, H), (B, H))]
    leaves = [seq.requires_grad_(True)] + make_params(D, H, device) + \
        [att.requires_grad_(True)]
    gru = torch.nn.GRU(D, H, batch_first=True).to(device).half()
    x = seq.detach()[..., :D].contiguous().requires_grad_(True)
    paths = {"eager": lambda: step(False, leaves, grads),
             "native": lambda: step(True, leaves, grads),
             "nn_gru": lambda: gru_step(gru, x, grads)}
    taken = {n: type(step(n == "native", leaves, grads)[1].grad_fn).__name__
             for n in ("eager", "native")}
    assert taken["native"] == "SeqGRUFnBackward" and taken["eager"] != taken["native"], taken
    for fn in paths.values():  # warm-up pass
        timed(fn, 3)
    names = ("states", "last", "dseq", "dWx", "dWh", "dbx", "dbh", "datt")
    diffs = [float((a - b).abs().max()) for a, b in
             zip(results(False, leaves, grads), results(True, leaves, grads))]
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            ms[name].append(timed(fn, steps))
    out = {"shape": dict(batch=B, sfs=L, max_len=max_len, dim=D, hidden=H,
                         valid_cells=cells, steps=steps, reps=reps)}
    for name in paths:
        out[name] = dict(
            ms_per_step_median=round(statistics.median(ms[name]), 4),
            ms_per_step_min=round(min(ms[name]), 4),
            ms_per_step_max=round(max(ms[name]), 4),
        )
    out["max_abs_diff"] = dict(zip(names, diffs))
    out["speedup_median"] = round(
        out["eager"]["ms_per_step_median"] / out["native"]["ms_per_step_median"], 3)
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
