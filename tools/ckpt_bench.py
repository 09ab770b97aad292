"""Checkpoint throughput: streaming dump/load of one HipEmbeddingStore to a
directory, end to end (device compaction -> pinned host -> file, and back).

The table is written directly (seeded keys and arena, no lookups): export
does not probe, and the load re-mixes every sign into its proper bucket.
Times are host wall-clock around work that ends in a device synchronize;
the dump time includes an fsync of the file, the load most likely reads
the page cache (the file was just written).  GB/s = file bytes / seconds.

With --legacy the whole-table path (PA_CKPT_STREAM=0) is timed too,
alternating with the streaming path in the same process — only at a size
where it still fits (it needs a second copy of every resident row in HBM
and several in host memory).

Run: python tools/ckpt_bench.py --slots 33554432 --dim 128 --occupancy 0.5 \\
         --dir /tmp/ckpt_bench [--legacy] [--repeats 3]
Prints one JSON line.
"""
import argparse
import json
import os
import shutil
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from persia_amd.core import checkpoint
from persia_amd.core.store import HipEmbeddingStore
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.optim import Adagrad


def fill(store, occupancy, seed):
    """Occupy ~occupancy of the slots with random keys; random rows."""
    g = torch.Generator(device=store.device).manual_seed(seed)
    step = 1 << 22
    for lo in range(0, store.n_slots, step):
        hi = min(store.n_slots, lo + step)
        keys = torch.randint(1, 1 << 62, (hi - lo,), generator=g,
                             device=store.device)
        keep = torch.rand(hi - lo, generator=g, device=store.device) < occupancy
        store.keys[lo:hi] = keys * keep
        store.arena[lo:hi].normal_(generator=g)
    store.ticks.zero_()


def shim(store):
    """The slice of an EmbeddingEngine that dump_embedding/load_embedding use."""
    eng = types.SimpleNamespace(
        dist=types.SimpleNamespace(rank=0, world_size=1),
        dist_grad=types.SimpleNamespace(barrier=lambda: None),
        stores={store.dim: store},
        progress=[],
    )
    eng._set_status = lambda status, pct=0.0: eng.progress.append(pct)
    return eng


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--occupancy", type=float, default=0.5)
    ap.add_argument("--dir", required=True)
    ap.add_argument("--legacy", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    store = HipEmbeddingStore(
        args.dim, args.slots, Adagrad(lr=0.01), EmbeddingConfig(), device
    )
    fill(store, args.occupancy, args.seed)
    rows = len(store)
    eng = shim(store)
    emb = os.path.join(args.dir, "s0", "replica_0_shard_0.emb")
    modes = ["stream", "legacy"] if args.legacy else ["stream"]
    res = {m: {"dump_s": [], "load_s": [], "rows_loaded": None} for m in modes}

    def dump():
        checkpoint.dump_embedding(eng, args.dir)
        fd = os.open(emb, os.O_RDONLY)
        os.fsync(fd)
        os.close(fd)

    # dumps first (the table is the seeded one for every repeat), then loads
    file_bytes = 0
    for _ in range(args.repeats):
        for m in modes:
            os.environ["PA_CKPT_STREAM"] = "1" if m == "stream" else "0"
            shutil.rmtree(args.dir, ignore_errors=True)
            os.makedirs(args.dir)
            res[m]["dump_s"].append(timed(dump))
            file_bytes = os.path.getsize(emb)
    for _ in range(args.repeats):
        for m in modes:
            os.environ["PA_CKPT_STREAM"] = "1" if m == "stream" else "0"
            store.clear()
            res[m]["load_s"].append(
                timed(lambda: checkpoint.load_embedding(eng, args.dir))
            )
            res[m]["rows_loaded"] = len(store)
    shutil.rmtree(args.dir, ignore_errors=True)

    gb = file_bytes / 1e9
    out = {
        "bench": "ckpt",
        "slots": store.n_slots,
        "dim": args.dim,
        "row_width": store.row_width,
        "occupancy": args.occupancy,
        "rows": rows,
        "arena_bytes": store.arena.numel() * 4,
        "file_bytes": file_bytes,
        "chunk_rows": checkpoint.chunk_rows_for(store.row_width),
        "repeats": args.repeats,
    }
    for m in modes:
        r = res[m]
        out[m] = {
            "dump_s": [round(t, 4) for t in r["dump_s"]],
            "load_s": [round(t, 4) for t in r["load_s"]],
            "dump_gbps": round(gb / min(r["dump_s"]), 3),
            "load_gbps": round(gb / min(r["load_s"]), 3),
            "rows_loaded": r["rows_loaded"],
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
