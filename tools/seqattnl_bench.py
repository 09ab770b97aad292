"""Streamed target-attention pooling benchmark: the eager torch chain, the
whole-sample kernels (csrc/seqattn.hip) where they take the shape, and the
streamed kernels (csrc/seqattnl.hip), alternating in one process.

Shapes (B, L, D): (4096, 200, 64) and (4096, 200, 128), which the short kernel
serves with one wave per block, and (1024, 1024, 64), which it refuses (eager
and long only).  Lengths are uniform in 0..1.6 L clipped to L, so full, partial
and empty samples all occur.  A step is forward plus backward from a fixed f16
output gradient, with gradients for both the query and the sequence.  "eager"
is what ``PA_SEQ_ATTN_LONG=0`` runs (ops/reference.py and the autograd backward
of each of its ops), "short" ``seq_attn_pool``, "long" ``seq_attn_pool_long``.

Each path first makes a warm-up pass, then ``--steps`` steps are timed with
device events, ending in a synchronise.  The paths alternate, and the whole
thing repeats ``--reps`` times for the spread.  Reported per path: the median
ms/step and its min/max over the repetitions; for the long kernels also the
bytes a step has to move (``min_bytes``: seq once forward and -- the second
pass counted as compulsory too -- twice backward, dseq written once, q / g /
out / dq) over the median time; and the largest difference of each native
path's out, dq and dseq from the eager path's at the timed size (both round
to f16).  A comparison counts only when the faster path's max lies below the
slower path's min (``long_faster_than``).  One JSON line per shape.

Run: python tools/seqattnl_bench.py [--steps 50] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from persia_amd.ops import native, seqattn, seqattnl
from seqattn_bench import make_inputs

SHAPES = [(4096, 200, 64), (4096, 200, 128), (1024, 1024, 64)]
NODES = {"short": "SeqAttnPoolFnBackward", "long": "SeqAttnPoolLongFnBackward"}


def step(path, q, seq, g):
    seqattnl._ENABLED = path == "long"  # what PA_SEQ_ATTN_LONG sets at import
    q.grad = seq.grad = None
    fn = seqattn.seq_attn_pool if path == "short" else seqattnl.seq_attn_pool_long
    out = fn(q, seq)
    out.backward(g)
    return out


def min_bytes(B, L, D):
    """seq once forward and twice backward, dseq out, and the five [B, D]
    tensors (q twice, g, out, dq), all f16."""
    return 2 * (4 * B * L * (D + 1) + 5 * B * D)


def results(path, q, seq, g):
    out = step(path, q, seq, g)
    return [t.detach().float() for t in (out, q.grad, seq.grad)]


def run(path, q, seq, g, steps):
    """-> ms/step by device events."""
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    ev0.record()
    for _ in range(steps):
        step(path, q, seq, g)
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps


def bench(shape, steps, reps, device):
    B, L, D = shape
    assert native().seq_attn_long_feasible(L, D), "no kernel for this shape"
    q, seq, g, cells = make_inputs(B, L, D, int(1.6 * L), device)
    q.requires_grad_(True)
    seq.requires_grad_(True)
    paths = ["eager", "long"]
    if native().seq_attn_feasible(L, D):
        paths.insert(1, "short")
    for path in paths:  # warm-up pass, and the path really taken
        node = type(step(path, q, seq, g).grad_fn).__name__
        assert node == NODES[path] if path in NODES else node not in NODES.values(), \
            (path, node)
        run(path, q, seq, g, 5)
    eager = results("eager", q, seq, g)
    diffs = {p: dict(zip(("out", "dq", "dseq"),
                         (float((a - b).abs().max())
                          for a, b in zip(results(p, q, seq, g), eager))))
             for p in paths[1:]}
    ms = {p: [] for p in paths}
    for _ in range(reps):
        for path in paths:
            ms[path].append(run(path, q, seq, g, steps))
    out = {"shape": dict(batch=B, L=L, dim=D, valid_cells=cells, steps=steps,
                         reps=reps)}
    for path in paths:
        out[path] = dict(ms_per_step_median=round(statistics.median(ms[path]), 4),
                         ms_per_step_min=round(min(ms[path]), 4),
                         ms_per_step_max=round(max(ms[path]), 4))
    out["long"]["min_bytes"] = min_bytes(B, L, D)
    out["long"]["gb_per_s_at_median"] = round(
        min_bytes(B, L, D) / out["long"]["ms_per_step_median"] / 1e6, 1)
    out["max_abs_diff_from_eager"] = diffs
    out["long_faster_than"] = [p for p in paths if p != "long" and
                               max(ms["long"]) < min(ms[p])]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    for shape in SHAPES:
        bench(shape, args.steps, args.reps, device)


if __name__ == "__main__":
    main()
