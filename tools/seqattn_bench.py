"""Target-attention pooling benchmark: the eager torch chain against the HIP
kernels (csrc/seqattn.hip), alternating in one process.

Shape: the raw slot of tools/raw_bench.py -- per-GPU batch 4096,
``sample_fixed_size`` 50, dim 64, lengths uniform in 0..80 clipped to 50 (so
full, partial and empty samples all occur) -- as the ``(B, L, D+1)`` f16
tensor ``prepare_features`` hands the model, and a ``(B, D)`` f16 query.  A
step is forward plus backward of ``seq_attn_pool`` from a fixed f16 output
gradient, with gradients for both the query and the sequence.  "eager" is
what ``PA_SEQ_ATTN=0`` runs (ops/reference.py: slice, masked scores, softmax,
weighted sum and the autograd backward of each), "native" one kernel per
direction.

Each path first makes a warm-up pass (kernel-module loads, allocator), then
``--steps`` steps are timed with device events, ending in a synchronise.  The
paths alternate, and the whole thing repeats ``--reps`` times for the spread.
Reported per path: the median ms/step and its min/max over the repetitions;
for the kernels also the bytes a step has to move (``min_bytes``: seq read
once per direction, dseq written once, q / g / out / dq) over the median time;
and the largest difference between the two paths' out, dq and dseq at the
timed size (both round to f16, so a few f16 ulps).  One JSON line.

Run: python tools/seqattn_bench.py [--steps 200] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from persia_amd.ops import native, seqattn


def make_inputs(B, L, D, max_len, device):
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(0, max_len + 1, (B,), generator=gen).clamp(max=L)
    mask = (torch.arange(L)[None, :] < lens[:, None]).half()
    rows = (torch.randn(B, L, D, generator=gen) * 0.5).half() * mask[..., None]
    seq = torch.cat([rows, mask[..., None]], dim=2).to(device)
    q = (torch.randn(B, D, generator=gen) * 0.5).half().to(device)
    g = (torch.randn(B, D, generator=gen) * 0.5).half().to(device)
    return q, seq, g, int(lens.sum())


def step(use_native, q, seq, g):
    seqattn._ENABLED = use_native  # what PA_SEQ_ATTN sets at import
    q.grad = seq.grad = None
    out = seqattn.seq_attn_pool(q, seq)
    out.backward(g)
    return out


def min_bytes(B, L, D):
    """What forward + backward must move: seq in each direction, dseq out,
    and the five [B, D] tensors (q twice, g, out, dq), all f16."""
    return 2 * (3 * B * L * (D + 1) + 5 * B * D)


def results(use_native, q, seq, g):
    out = step(use_native, q, seq, g)
    return [t.detach().float() for t in (out, q.grad, seq.grad)]


def run(use_native, q, seq, g, steps):
    """-> ms/step by device events."""
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    ev0.record()
    for _ in range(steps):
        step(use_native, q, seq, g)
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sfs", type=int, default=50)
    ap.add_argument("--max-len", type=int, default=80)
    ap.add_argument("--dim", type=int, default=64)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    assert native().seq_attn_feasible(args.sfs, args.dim), "no kernel for this shape"
    q, seq, g, cells = make_inputs(args.batch, args.sfs, args.dim, args.max_len,
                                   device)
    q.requires_grad_(True)
    seq.requires_grad_(True)
    paths = {"eager": False, "native": True}
    taken = {}
    for name, use_native in paths.items():  # warm-up pass
        taken[name] = type(step(use_native, q, seq, g).grad_fn).__name__
        run(use_native, q, seq, g, 10)
    assert taken["native"] == "SeqAttnPoolFnBackward", taken
    assert taken["eager"] != taken["native"], taken
    diffs = [float((a - b).abs().max()) for a, b in
             zip(results(False, q, seq, g), results(True, q, seq, g))]
    ms = {k: [] for k in paths}
    for _ in range(args.reps):
        for name, use_native in paths.items():
            ms[name].append(run(use_native, q, seq, g, args.steps))
    out = {"shape": dict(batch=args.batch, sfs=args.sfs, max_len=args.max_len,
                         dim=args.dim, valid_cells=cells, steps=args.steps,
                         reps=args.reps)}
    for name in paths:
        out[name] = dict(
            ms_per_step_median=round(statistics.median(ms[name]), 4),
            ms_per_step_min=round(min(ms[name]), 4),
            ms_per_step_max=round(max(ms[name]), 4),
        )
    nbytes = min_bytes(args.batch, args.sfs, args.dim)
    out["native"]["min_bytes"] = nbytes
    out["native"]["gb_per_s_at_median"] = round(
        nbytes / out["native"]["ms_per_step_median"] / 1e6, 1)
    out["max_abs_diff"] = dict(zip(("out", "dq", "dseq"), diffs))
    out["speedup_median"] = round(
        out["eager"]["ms_per_step_median"] / out["native"]["ms_per_step_median"],
        3,
    )
    print(json.dumps(out))


if __name__ == "__main__":
    main()
