"""Raw (sequence) slot lookup + update benchmark: the generic path against the
native raw path, alternating in one process.

Shape: 24 single-ID sum slots plus 2 raw history slots with
``sample_fixed_size`` 50 and lengths uniform in 0..80 (so truncation and
padding both happen), dim 64, per-GPU batch 4096, ids over 1e6 rows per slot,
one GPU.  A step is ``process_batch``, the model-input tensors that
``prepare_features`` builds for the raw slots, the gradient that
``TrainCtx._on_backward`` builds from a fixed f16 cell gradient, and
``apply_gradients_base``.  On the raw path the input is one ``cat`` and
there is no per-slot gradient to build; on the generic path it is the
``index_select`` / compare / ``cat`` chain and the ``index_add_`` scatter, and
the whole batch leaves the fused update.  Nothing else of the engine is used,
so the script also runs on a tree without the raw path (both engines then take
the generic one).

Each engine first makes one pass over the batch pool (inserts, pinned staging,
kernel-module loads), then ``--steps`` steps are timed with device events,
ending in a synchronise.  The engines alternate (PA_RAW_FAST=0, then on), and
the whole thing repeats ``--reps`` times for the spread.  Reported per engine:
the median ms/step and its min/max over the repetitions, and the
producer-thread time per batch (PA_PROD_TIMING: host time inside
``process_batch``).  One JSON line.

Run: python tools/raw_bench.py [--steps 200] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from persia_amd.core.comm import DistContext
from persia_amd.core.engine import EmbeddingEngine
from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.data import (
    IDTypeFeatureWithSingleID, Label, PersiaBatch, _FlatIDFeature,
)
from persia_amd.embedding.optim import Adagrad


def make_batch(seed, n_sum, n_raw, B, vocab, max_len):
    """Single-ID sum slots f*, raw slots h* built straight in CSR form."""
    rng = np.random.default_rng(seed)
    feats = [
        IDTypeFeatureWithSingleID(
            f"f{i}", rng.integers(0, vocab, size=B, dtype=np.uint64))
        for i in range(n_sum)
    ]
    batch = PersiaBatch(
        feats + [IDTypeFeatureWithSingleID(f"h{i}", np.zeros(B, np.uint64))
                 for i in range(n_raw)],
        labels=[Label(np.ones((B, 1), np.float32))], requires_grad=True,
    )
    feats = batch.id_type_features[:n_sum]  # flattened by PersiaBatch
    for i in range(n_raw):
        lens = rng.integers(0, max_len + 1, size=B)
        offsets = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        values = rng.integers(0, vocab, size=int(offsets[-1]), dtype=np.uint64)
        feats.append(_FlatIDFeature(f"h{i}", values, offsets))
    batch.id_type_features = feats
    return batch


def make_engine(raw_fast, n_sum, n_raw, sfs, dim, capacity, device):
    os.environ["PA_RAW_FAST"] = "1" if raw_fast else "0"
    os.environ["PA_PROD_TIMING"] = "1"
    slots = {f"f{i}": SlotConfig(name=f"f{i}", dim=dim) for i in range(n_sum)}
    slots.update({
        f"h{i}": SlotConfig(name=f"h{i}", dim=dim, embedding_summation=False,
                            sample_fixed_size=sfs)
        for i in range(n_raw)
    })
    eng = EmbeddingEngine(
        schema=EmbeddingSchema(slots=slots, feature_index_prefix_bit=8),
        hyper=EmbeddingConfig(), optimizer=Adagrad(lr=0.01),
        gconf=GlobalConfig(capacity=capacity), device=device,
        dist_ctx=DistContext(1, 0),
    )
    eng._pt["skip"] = 0  # the warm-up pass is excluded by snapshots instead
    return eng


_GBASE = {}


def step(eng, batch, sum_grad, cell_grad):
    """Lookup, the raw slots' model inputs and gradients as the ctx builds
    them, update.  -> the inputs (kept alive until the update is issued)."""
    tb = eng.process_batch(batch)
    B = tb.batch_size
    inputs, raw_grads = [], {}
    for p in tb.payloads:
        if getattr(p, "raw_rows", None) is not None:
            inputs.append(torch.cat([p.raw_rows, p.raw_mask], dim=2))
        elif p.is_raw:
            sfs = p.raw_index.shape[-1] // B
            sel = p.raw_distinct.index_select(0, p.raw_index.view(-1))
            mask = (p.raw_index.view(B, sfs, 1) != 0).half()
            inputs.append(torch.cat([sel.view(B, sfs, -1), mask], dim=2))
            grad = torch.zeros_like(p.raw_distinct, dtype=torch.float32)
            nz = p.raw_non_empty_index.view(-1)
            grad.index_add_(0, p.raw_index.view(-1)[nz],
                            cell_grad.index_select(0, nz).float())
            raw_grads[p.name] = grad[1:, :]
    # the gradient of the group's base: the sum rows, and on the raw path the
    # raw slots' cell rows behind them (built once per shape)
    n_rows = tb._groups[0].sum_base.shape[0]
    gbase = _GBASE.get(n_rows)
    if gbase is None:
        n_raw = (n_rows - sum_grad.shape[0]) // cell_grad.shape[0]
        gbase = _GBASE[n_rows] = torch.cat([sum_grad] + [cell_grad] * n_raw)
    eng.apply_gradients_base(tb, raw_grads, sum_base_grads=[gbase])
    return inputs


def run(eng, pool, sum_grad, cell_grad, steps):
    """-> (ms/step by device events, producer ms/batch) of `steps` steps."""
    t_host0, n0 = eng._pt["batch"], eng._pt["n"]
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    ev0.record()
    for i in range(steps):
        step(eng, pool[i % len(pool)], sum_grad, cell_grad)
    ev1.record()
    torch.cuda.synchronize()
    prod = (eng._pt["batch"] - t_host0) / max(1, eng._pt["n"] - n0)
    return ev0.elapsed_time(ev1) / steps, prod * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sum-slots", type=int, default=24)
    ap.add_argument("--raw-slots", type=int, default=2)
    ap.add_argument("--sfs", type=int, default=50)
    ap.add_argument("--max-len", type=int, default=80)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=1 << 23)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    pool = [make_batch(s, args.sum_slots, args.raw_slots, args.batch,
                       args.vocab, args.max_len) for s in range(args.pool)]
    nnz = [sum(len(f.values) for f in b.id_type_features) for b in pool]
    sum_grad = torch.full((args.sum_slots * args.batch, args.dim), 1e-3,
                          dtype=torch.float16, device=device)
    cell_grad = torch.full((args.batch * args.sfs, args.dim), 1e-3,
                           dtype=torch.float16, device=device)
    shape = (args.sum_slots, args.raw_slots, args.sfs, args.dim,
             args.capacity, device)
    engines = {"generic": make_engine(False, *shape),
               "raw": make_engine(True, *shape)}
    for eng in engines.values():
        run(eng, pool, sum_grad, cell_grad, len(pool))  # warm-up pass
    ms = {k: [] for k in engines}
    prod = {k: [] for k in engines}
    for _ in range(args.reps):
        for name, eng in engines.items():
            m, p = run(eng, pool, sum_grad, cell_grad, args.steps)
            ms[name].append(m)
            prod[name].append(p)
    out = {
        "shape": dict(sum_slots=args.sum_slots, raw_slots=args.raw_slots,
                      sfs=args.sfs, max_len=args.max_len, dim=args.dim,
                      batch=args.batch, vocab=args.vocab,
                      mean_nnz=int(np.mean(nnz)), steps=args.steps,
                      reps=args.reps),
        "raw_path_taken": bool(getattr(engines["raw"], "_raw_fast", False)),
    }
    for name in engines:
        out[name] = dict(
            ms_per_step_median=round(statistics.median(ms[name]), 4),
            ms_per_step_min=round(min(ms[name]), 4),
            ms_per_step_max=round(max(ms[name]), 4),
            producer_ms_per_batch_median=round(
                statistics.median(prod[name]), 4),
        )
    out["speedup_median"] = round(
        out["generic"]["ms_per_step_median"] / out["raw"]["ms_per_step_median"],
        3,
    )
    print(json.dumps(out))


if __name__ == "__main__":
    main()
