"""Activation-unit (MLP attention) pooling benchmark: the eager torch chain
against the HIP kernels (csrc/actunit.hip), alternating in one process.

Shapes: the raw slot of tools/raw_bench.py -- per-GPU batch 4096,
``sample_fixed_size`` 50, dim 64, lengths uniform in 0..80 clipped to the
slot's size -- with 32 hidden units, and once a long one (``sample_fixed_size``
200, dim 128, 64 hidden units, lengths 0..320).  A step is forward plus
backward of ``act_unit_pool`` from a fixed f16 output gradient with gradients
for the query, the sequence and all four parameters.  "eager" is what
``PA_ACT_UNIT=0`` runs (ops/reference.py on the GPU, f32 arithmetic on the f16
tensors), "native" the kernels plus the addmm for u.

Each path first makes a warm-up pass, then ``--steps`` steps are timed with
device events, ending in a synchronise.  The paths alternate, and the whole
thing repeats ``--reps`` times for the spread.  Reported per shape and path:
the median ms/step and its min/max over the repetitions, and the largest
difference between the two paths' results.  One JSON line per shape.

Run: python tools/actunit_bench.py [--steps 100] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from persia_amd.ops import actunit
from seqattn_bench import make_inputs

SHAPES = [(4096, 50, 64, 32, 80), (4096, 200, 128, 64, 320)]  # B, L, D, H, max_len


def make_params(D, H, device):
    gen = torch.Generator().manual_seed(1)
    W1 = torch.randn(H, 4 * D, generator=gen) * (0.5 * D ** -0.5)
    b1, w2 = torch.randn(H, generator=gen) * 0.1, torch.randn(H, generator=gen) * 0.5
    b2 = torch.randn((), generator=gen) * 0.1
    return [p.to(device).requires_grad_(True) for p in (W1, b1, w2, b2)]


def step(use_native, leaves, g):
    actunit._ENABLED = use_native  # what PA_ACT_UNIT sets at import
    for t in leaves:
        t.grad = None
    out = actunit.act_unit_pool(*leaves)
    out.backward(g)
    return out


def results(use_native, leaves, g):
    out = step(use_native, leaves, g)
    return [out.detach().float()] + [t.grad.detach().float() for t in leaves]


def run(use_native, leaves, g, steps):
    """-> ms/step by device events."""
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    ev0.record()
    for _ in range(steps):
        step(use_native, leaves, g)
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps


def bench(shape, steps, reps, device):
    B, L, D, H, max_len = shape
    q, seq, g, cells = make_inputs(B, L, D, max_len, device)
    leaves = [q.requires_grad_(True), seq.requires_grad_(True)] + make_params(D, H, device)
    paths = {"eager": False, "native": True}
    taken = {}
    for name, use_native in paths.items():  # warm-up pass
        taken[name] = type(step(use_native, leaves, g).grad_fn).__name__
        run(use_native, leaves, g, 5)
    assert taken["native"] == "ActUnitPoolFnBackward", taken
    assert taken["eager"] != taken["native"], taken
    names = ("out", "dq", "dseq", "dW1", "db1", "dw2", "db2")
    diffs = [float((a - b).abs().max()) for a, b in
             zip(results(False, leaves, g), results(True, leaves, g))]
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for name, use_native in paths.items():
            ms[name].append(run(use_native, leaves, g, steps))
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
