"""Multi-hot (embedding-bag) lookup + update benchmark: the generic path
against the native bag path, alternating in one process.

Shape: 26 sum slots, dim 128, per-GPU batch 8192, bag lengths from a seeded
geometric distribution (mean about 4, clipped at 30, empty bags included),
ids over 1e6 rows per slot, one GPU.  A step is ``process_batch`` plus
``apply_gradients_base`` with a fixed gradient -- nothing else of the engine
is used, so the script also runs on a tree without the bag path (both engines
then take the generic one).

Each engine first makes one pass over the batch pool (inserts, pinned
staging, kernel-module loads), then ``--steps`` steps are timed with device
events, ending in a synchronise.  The engines alternate (PA_BAG_FAST=0, then
on), and the whole thing repeats ``--reps`` times for the spread.  Reported
per engine: the median ms/step and its min/max over the repetitions, and the
producer-thread time per batch (PA_PROD_TIMING: host time inside
``process_batch``).  One JSON line.

``--optimizer`` picks the embedding optimizer (default adagrad); adam and ftrl
move three vectors per column where adagrad moves two.

``--hashstack ROUNDS:SIZE`` gives every slot a ``hash_stack_config`` of ROUNDS
rounds over SIZE buckets (default: none), so each id becomes ROUNDS positions;
``mean_nnz`` in the result stays the number of ids, ``mean_positions`` is the
expanded count.

Run: python tools/bag_bench.py [--steps 200] [--reps 3]
         [--optimizer {sgd,adagrad,adam,ftrl}] [--hashstack ROUNDS:SIZE]
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
from persia_amd.core.schema import (
    EmbeddingSchema, GlobalConfig, HashStackConfig, SlotConfig,
)
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.data import (
    IDTypeFeatureWithSingleID, Label, PersiaBatch, _FlatIDFeature,
)
from persia_amd.embedding import optim


def make_batch(seed, n_slots, B, vocab, mean_len, max_len):
    """Bag slots built straight in CSR form (B*n_slots per-sample arrays
    would take seconds per batch to build)."""
    rng = np.random.default_rng(seed)
    names = [f"f{i}" for i in range(n_slots)]
    batch = PersiaBatch(
        [IDTypeFeatureWithSingleID(n, np.zeros(B, dtype=np.uint64))
         for n in names],
        labels=[Label(np.ones((B, 1), np.float32))], requires_grad=True,
    )
    feats = []
    for n in names:
        lens = np.minimum(rng.geometric(1.0 / (mean_len + 1), size=B) - 1,
                          max_len)
        offsets = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        values = rng.integers(0, vocab, size=int(offsets[-1]), dtype=np.uint64)
        feats.append(_FlatIDFeature(n, values, offsets))
    batch.id_type_features = feats
    return batch


def make_optimizer(name):
    if name == "sgd":
        return optim.SGD(lr=0.01)
    if name == "adagrad":
        return optim.Adagrad(lr=0.01)
    if name == "adam":
        return optim.Adam(lr=0.001)
    return optim.Ftrl(lr=0.05, beta=1.0, l1=1e-4, l2=1e-4)


def parse_hashstack(text):
    """"ROUNDS:SIZE" -> (rounds, size), both at least 1."""
    rounds, _, size = text.partition(":")
    try:
        rounds, size = int(rounds), int(size)
    except ValueError:
        rounds = size = 0
    if rounds < 1 or size < 1:
        raise argparse.ArgumentTypeError(
            f"{text!r}: expected ROUNDS:SIZE, two integers of at least 1")
    return rounds, size


def make_engine(bag_fast, n_slots, dim, capacity, device, optimizer="adagrad",
                hashstack=None):
    os.environ["PA_BAG_FAST"] = "1" if bag_fast else "0"
    os.environ["PA_PROD_TIMING"] = "1"
    stack = {}
    if hashstack:
        stack = dict(hash_stack_config=HashStackConfig(
            hash_stack_rounds=hashstack[0], embedding_size=hashstack[1]))
    schema = EmbeddingSchema(
        slots={f"f{i}": SlotConfig(name=f"f{i}", dim=dim, **stack)
               for i in range(n_slots)},
        feature_index_prefix_bit=8,
    )
    eng = EmbeddingEngine(
        schema=schema, hyper=EmbeddingConfig(),
        optimizer=make_optimizer(optimizer),
        gconf=GlobalConfig(capacity=capacity), device=device,
        dist_ctx=DistContext(1, 0),
    )
    eng._pt["skip"] = 0  # the warm-up pass is excluded by snapshots instead
    return eng


def run(eng, pool, grad, steps):
    """-> (ms/step by device events, producer ms/batch) of `steps` steps."""
    t_host0, n0 = eng._pt["batch"], eng._pt["n"]
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    ev0.record()
    for i in range(steps):
        tb = eng.process_batch(pool[i % len(pool)])
        eng.apply_gradients_base(tb, sum_base_grads=[grad])
    ev1.record()
    torch.cuda.synchronize()
    prod = (eng._pt["batch"] - t_host0) / max(1, eng._pt["n"] - n0)
    return ev0.elapsed_time(ev1) / steps, prod * 1e3


def path_taken(eng, batch):
    """Whether the engine sends the batch's groups down the bag path (a tree
    without that path has no ``_bag_group``)."""
    if not hasattr(eng, "_bag_group"):
        return False
    return all(eng._bag_group(d, f)
               for d, f in eng._feats_by_dim(batch).items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=26)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=1 << 23)
    ap.add_argument("--optimizer", default="adagrad",
                    choices=["sgd", "adagrad", "adam", "ftrl"])
    ap.add_argument("--hashstack", type=parse_hashstack, default=None,
                    metavar="ROUNDS:SIZE")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    pool = [make_batch(s, args.slots, args.batch, args.vocab, 4, 30)
            for s in range(args.pool)]
    nnz = [sum(len(f.values) for f in b.id_type_features) for b in pool]
    grad = torch.full((args.slots * args.batch, args.dim), 1e-3,
                      dtype=torch.float16, device=device)
    engines = {
        "generic": make_engine(False, args.slots, args.dim, args.capacity,
                               device, args.optimizer, args.hashstack),
        "bag": make_engine(True, args.slots, args.dim, args.capacity, device,
                           args.optimizer, args.hashstack),
    }
    for eng in engines.values():
        run(eng, pool, grad, len(pool))  # warm-up: one pass over the pool
    ms = {k: [] for k in engines}
    prod = {k: [] for k in engines}
    for _ in range(args.reps):
        for name, eng in engines.items():
            m, p = run(eng, pool, grad, args.steps)
            ms[name].append(m)
            prod[name].append(p)
    out = {
        "shape": dict(slots=args.slots, dim=args.dim, batch=args.batch,
                      vocab=args.vocab, mean_nnz=int(np.mean(nnz)),
                      steps=args.steps, reps=args.reps,
                      optimizer=args.optimizer),
        "bag_path_taken": path_taken(engines["bag"], pool[0]),
    }
    if args.hashstack:
        out["shape"]["hashstack"] = "%d:%d" % args.hashstack
        out["shape"]["mean_positions"] = int(np.mean(nnz)) * args.hashstack[0]
    for name in engines:
        out[name] = dict(
            ms_per_step_median=round(statistics.median(ms[name]), 4),
            ms_per_step_min=round(min(ms[name]), 4),
            ms_per_step_max=round(max(ms[name]), 4),
            producer_ms_per_batch_median=round(
                statistics.median(prod[name]), 4),
        )
    out["speedup_median"] = round(
        out["generic"]["ms_per_step_median"] / out["bag"]["ms_per_step_median"],
        3,
    )
    print(json.dumps(out))


if __name__ == "__main__":
    main()
