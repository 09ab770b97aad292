"""The DCN-v2 low-rank cross stack alone: the fused op (ops.cross.cross_stack,
csrc/cross.hip) against the present chain of ``CrossLayerV2(fused=True)`` on
the same parameters, alternating in one process.

Shapes: the ``dcn-spill`` tower (B 8192, D 1696, rank 256, 3 layers) and the
same tower at rank 64.  A step is forward plus backward from a fixed bf16
gradient, with gradients for ``x0`` and every parameter (bf16 weights, f32
biases, as ``DCNv2(fused=True).bfloat16()`` holds them).

Both paths are warmed up, then ``--steps`` steps are timed with device events,
ending in a synchronise.  The paths alternate and the whole thing repeats
``--reps`` times; reported per shape and path: ms/step min, median and max
over the repetitions, whether the fused maximum lies below the chain's
minimum, and the [B, D] bf16 traffic per layer computed from the shapes
(passes over HBM, forward: 10 for the chain, 4 fused).  One JSON line per
shape.  Needs a GPU; exits non-zero otherwise.

Run: python tools/cross_bench.py [--steps 100] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from persia_amd.models.dcn import CrossLayerV2
from persia_amd.ops.cross import cross_stack

SHAPES = [(8192, 1696, 256, 3), (8192, 1696, 64, 3)]  # B D r layers
FWD_PASSES = {"chain": 10, "fused": 4}  # [B, D] bf16 passes per layer


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
    B, D, r, n = shape
    torch.manual_seed(3)
    layers = torch.nn.ModuleList(
        [CrossLayerV2(D, rank=r, fused=True) for _ in range(n)]).bfloat16().to(device)
    for layer in layers:
        torch.nn.init.normal_(layer.u.bias, std=r ** -0.5)
    gen = torch.Generator().manual_seed(4)
    x0 = torch.randn(B, D, generator=gen).bfloat16().to(device).requires_grad_(True)
    g = torch.randn(B, D, generator=gen).bfloat16().to(device)
    params = list(layers.parameters())

    def chain():
        xl = x0
        for layer in layers:
            xl = layer(x0, xl)
        return xl

    def fused():
        return cross_stack(x0, [l.v.weight for l in layers],
                           [l.u.weight for l in layers],
                           [l.u.bias for l in layers])

    def step(fn):
        for t in (x0, *params):
            t.grad = None
        out = fn()
        out.backward(g)
        return out

    paths = {"chain": lambda: step(chain), "fused": lambda: step(fused)}
    assert type(fused().grad_fn).__name__ == "CrossStackFnBackward"
    for fn in paths.values():  # warm-up pass
        timed(fn, 3)
    res = {}
    for name, fn in paths.items():
        out = fn().detach().float()
        res[name] = [out, x0.grad.float()] + [p.grad.float() for p in params]
    diffs = [float((p - q).abs().max() / q.abs().max().clamp_min(1e-30))
             for p, q in zip(res["fused"], res["chain"])]
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            ms[name].append(timed(fn, steps))
    out = {"shape": dict(batch=B, width=D, rank=r, layers=n, steps=steps, reps=reps)}
    for name in paths:
        out[name] = dict(
            ms_per_step_min=round(min(ms[name]), 4),
            ms_per_step_median=round(statistics.median(ms[name]), 4),
            ms_per_step_max=round(max(ms[name]), 4),
            fwd_bd_bytes_per_layer=FWD_PASSES[name] * B * D * 2,
        )
    out["fused_max_below_chain_min"] = max(ms["fused"]) < min(ms["chain"])
    out["max_diff_over_max_abs"] = dict(out=diffs[0], dx0=diffs[1],
                                        params=max(diffs[2:]))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    for shape in SHAPES:
        bench(shape, args.steps, args.reps, device)


if __name__ == "__main__":
    main()
