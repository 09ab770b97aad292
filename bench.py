"""Flagship benchmark: DLRM-Criteo-shape hybrid training throughput.

BASELINE.json metric: samples/sec (whole node) for a DLRM-style model —
26 sparse slots (1e8-row ID space, dim=128, embeddings resident in HBM as a
sharded hash table), 13 dense features, synthetic uniform ID/label data,
random-init weights, bf16 dense compute, f16 embedding wire, Adagrad sparse
optimizer, bounded-staleness async sparse pipeline + DDP dense.

Contract (driver):
  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
N>1 is launched via torch.distributed.run (one rank per GPU over RCCL);
weak scaling (per-GPU batch fixed).  Rank 0 prints ONE json line.

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, optionally dump the last step's outputs, print the result line.
--full is reserved for measurements beyond the headline figure (baselines,
other configurations, comparisons); there are none today, so it currently
runs the same steps as a plain run.
"""
import argparse
import json
import os
import time

import numpy as np
import torch


# The five BASELINE.json configs. "criteo" is the headline.
PRESETS = {
    "ctr-smoke": dict(model="dlrm", num_sparse=2, num_dense=5, dim=8, rows=2e4,
                      batch_size=128),
    "criteo": dict(model="dlrm", num_sparse=26, num_dense=13, dim=128, rows=1e8),
    "terabyte": dict(model="dlrm", num_sparse=26, num_dense=13, dim=128, rows=1e10),
    # sparse_priority=-1: dcn is sparse-stream-critical; raising that
    # stream's priority measured 2.67 -> 2.98M (neutral on criteo, slightly
    # negative on terabyte).  After the side-band flat-gradient scheme the
    # fused dense path wins on EVERY preset (dcn 3.0 -> 3.26M, 100t
    # 5.25 -> 5.56M re-measured same box).
    "dcn-spill": dict(model="dcn", num_sparse=26, num_dense=13, dim=64, rows=1e11,
                      spill_capacity=2e8, sparse_priority=-1),
    "100t": dict(model="dlrm", num_sparse=64, num_dense=13, dim=8, rows=1e12),
}


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--preset", type=str, default="criteo", choices=list(PRESETS))
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch-size", type=int, default=None, help="per-GPU batch")
    p.add_argument("--num-sparse", type=int, default=None)
    p.add_argument("--num-dense", type=int, default=None)
    p.add_argument("--dim", type=int, default=None)
    p.add_argument("--rows", type=float, default=None, help="total ID space")
    p.add_argument("--capacity", type=float, default=None,
                   help="resident rows per rank (default: min(rows/world, HBM budget))")
    p.add_argument("--hbm-budget-gb", type=float, default=200.0,
                   help="HBM bytes budget for the table per rank")
    p.add_argument("--spill-capacity", type=float, default=None,
                   help="host-DRAM rows per rank (0 = off)")
    p.add_argument("--staleness", type=int, default=8)
    p.add_argument("--model", type=str, default=None, choices=["dlrm", "dcn"])
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--graph", type=int, default=1,
                   help="capture dense fwd+bwd in a hipGraph (1 GPU only)")
    p.add_argument("--sparse-priority", type=int, default=None,
                   help="lookup-stream priority (-1 = high; preset default)")
    p.add_argument("--flat-params", type=int, default=None,
                   help="flat param/grad/master buffers in the graphed step "
                        "(preset-dependent default)")
    p.add_argument("--fused-dense", type=int, default=None,
                   help="use the hand-written MFMA GEMM+bias+ReLU layers "
                        "(beats the graphed hipBLASLt path since the "
                        "XOR-swizzled staging fixed wgrad; 0 = hipBLASLt; "
                        "preset-dependent default)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step computed (loss, logits, dense parameters and "
                        "seeded samples of the embedding sums and their "
                        "gradient) as DIR/<name>.npy in float32")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline "
                        "figure (none today: same as a plain run)")
    args = p.parse_args()
    preset = dict(PRESETS[args.preset])
    preset.setdefault("batch_size", 8192)  # x8 ranks = the MLPerf DLRM 64k global batch
    preset.setdefault("spill_capacity", 0)
    preset.setdefault("fused_dense", 1)
    preset.setdefault("flat_params", 1)
    preset.setdefault("sparse_priority", 0)
    for k, v in preset.items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    return args


def _self_launch(args):
    """Re-exec under torch.distributed.run when --gpus N (N>1) is given
    directly (no torchrun env present): one rank per GPU over RCCL.  The
    child ranks inherit the full original argv; their RANK/WORLD_SIZE env
    stops the recursion.  Propagates the child's stdout (rank 0 prints the
    JSON line) and exit code."""
    import socket
    import subprocess
    import sys

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", f"--nproc-per-node={args.gpus}",
        "--master-addr=127.0.0.1", f"--master-port={port}",
        os.path.abspath(__file__), *sys.argv[1:],
    ]
    raise SystemExit(subprocess.call(cmd))


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _self_launch(args)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    use_gpu = torch.cuda.is_available() and args.device != "cpu"
    if use_gpu:
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    else:
        device = torch.device("cpu")

    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group("nccl" if use_gpu else "gloo", rank=rank, world_size=world)

    if args.sparse_priority:
        os.environ.setdefault("PA_SPARSE_PRIORITY", str(args.sparse_priority))

    from persia_amd.core.comm import DistContext
    from persia_amd.core.engine import EmbeddingEngine, ForwardPipeline
    from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
    from persia_amd.embedding import EmbeddingConfig
    from persia_amd.embedding.data import IDTypeFeatureWithSingleID, Label, PersiaBatch
    from persia_amd.embedding.optim import Adagrad
    from persia_amd.models import DCNv2, DLRM

    n_slots, dim, B = args.num_sparse, args.dim, args.batch_size
    rows_total = int(args.rows)
    vocab_per_slot = max(1, rows_total // n_slots)
    # Adagrad doubles the row (dim emb + dim accumulator) + 12B key/tick
    hbm_rows = int(args.hbm_budget_gb * 1e9 / (dim * 2 * 4 + 12))
    capacity = (
        int(args.capacity) if args.capacity
        else max(1 << 20, min(rows_total // world, hbm_rows))
    )

    schema = EmbeddingSchema(
        slots={f"f{i}": SlotConfig(name=f"f{i}", dim=dim) for i in range(n_slots)},
        feature_index_prefix_bit=8,
    )
    engine = EmbeddingEngine(
        schema=schema,
        hyper=EmbeddingConfig(),
        optimizer=Adagrad(lr=0.01),
        gconf=GlobalConfig(
            capacity=capacity, spill_capacity=int(args.spill_capacity or 0)
        ),
        device=device,
        dist_ctx=DistContext.new_sparse_group(),
    )
    # same dense init on every run and rank (the host batches are seeded
    # below): two builds given the same arguments see identical inputs
    torch.manual_seed(1234)
    if args.model == "dlrm":
        model = DLRM(
            num_sparse=n_slots, num_dense=args.num_dense, dim=dim,
            fused=bool(args.fused_dense) and use_gpu,
        ).to(device)
    else:
        model = DCNv2(
            num_sparse=n_slots, num_dense=args.num_dense, dim=dim,
            fused=bool(args.fused_dense) and use_gpu,
        ).to(device)
    # bf16 model weights + f32 master weights (see the graph block below):
    # must happen BEFORE the DDP wrap so the gradient buckets are built bf16
    # (halves allreduce bytes over xGMI as a bonus)
    bf16_weights = (
        bool(args.graph) and use_gpu
        and os.environ.get("PA_GRAPH_BF16", "1") == "1"
    )
    if bf16_weights:
        model.bfloat16()
    # world>1 graph mode: do NOT capture RCCL inside the graph (unproven and
    # a capture hang would sink the whole run).  Instead the graph covers
    # fwd+bwd with gradients accumulating into ONE flat bf16 buffer; a single
    # plain all_reduce runs between the two graphs per step (a few MB over
    # xGMI).  DDP is only constructed for the eager fallback.
    defer_ddp = bool(args.graph) and use_gpu and world > 1 and bf16_weights

    def _wrap_ddp(m):
        from torch.nn.parallel import DistributedDataParallel

        return DistributedDataParallel(
            m,
            device_ids=[local_rank] if use_gpu else None,
            gradient_as_bucket_view=True,
            bucket_cap_mb=50,
        )

    if world > 1 and not defer_ddp:
        model = _wrap_ddp(model)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    if use_gpu:
        from persia_amd.ops.dense import fused_bce_with_logits as loss_fn
    else:
        loss_fn = torch.nn.functional.binary_cross_entropy_with_logits

    # ---- synthetic data: pre-generate host batches (excluded from timing)
    n_batches = args.steps + args.warmup
    rng = np.random.default_rng(1234 + rank)
    host_batches = []
    for _ in range(min(n_batches, 16)):
        feats = [
            IDTypeFeatureWithSingleID(
                f"f{i}",
                (rng.integers(0, vocab_per_slot, size=B, dtype=np.uint64)),
            )
            for i in range(n_slots)
        ]
        dense = rng.normal(size=(B, args.num_dense)).astype(np.float32)
        label = rng.integers(0, 2, size=(B,)).astype(np.float32)
        host_batches.append(
            PersiaBatch(
                feats,
                non_id_type_features=[dense],
                labels=[Label(label)],
                requires_grad=True,
            )
        )

    # pinned staging built up-front (setup, untimed): first-visit
    # hipHostMalloc in the pipeline thread is ms-scale on a freshly
    # reclaimed host and would dominate short runs
    for hb in host_batches:
        engine.prepare_host_batch(hb)

    if world > 1:
        # Serialize communicator creation: the default group (dense), the
        # sparse a2a group (pipeline thread) and the grad group (main
        # thread) all lazily build their NCCL communicator at first use —
        # two ranks initializing different comms concurrently from
        # different threads can deadlock.  One tiny collective per group,
        # one thread, fixed order.
        warm = torch.ones(1, device=device if use_gpu else None)
        dist.all_reduce(warm)
        engine.dist.barrier()
        engine.dist_grad.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    pipeline = ForwardPipeline(engine, staleness=args.staleness, out_buffer=args.staleness + 2)
    pipeline.start()

    amp_dtype = torch.bfloat16
    # cache_enabled=False: required for hipGraph capture of autocast regions
    amp_ctx = (
        torch.autocast("cuda", dtype=amp_dtype, cache_enabled=False)
        if use_gpu
        else _nullcontext()
    )

    # the flagship path feeds the model the PACKED per-group sum tensor
    # ([S*B, dim] slot-major) — one reshape in the model, gradients land in
    # sum_base.grad with no per-slot autograd traffic.  The whole dense
    # iteration (zero-grads + fwd + bwd + SGD step) is captured into ONE
    # hipGraph with static in/out buffers; each step copies inputs in and
    # replays (the dense side was launch-bound, ~200 kernels/step).
    graph = None
    graph_upd = None
    flat_grads = None
    static = {}
    if args.graph and use_gpu and (world == 1 or defer_ddp):
        try:
            # pre-pad + pre-cast the static dense input for the fused DLRM:
            # the fused layers zero-pad K to %128 per step anyway (inert zero
            # columns hit zero-padded weight columns), so a statically padded
            # bf16 buffer kills that pad pass and the per-step f32->bf16 cast
            nd = args.num_dense
            d_dtype = torch.float32
            if args.model == "dlrm" and bool(args.fused_dense) and bf16_weights:
                nd = (args.num_dense + 127) // 128 * 128
                d_dtype = torch.bfloat16
            static = {
                "dense": torch.zeros(B, nd, dtype=d_dtype, device=device),
                "base": torch.zeros(
                    n_slots * B, dim, dtype=torch.float16, device=device,
                    requires_grad=True,
                ),
                "label": torch.zeros(B, device=device),
            }
            # bf16 model weights + f32 master weights: autocast with
            # cache_enabled=False (required for capture) re-casts every
            # weight on every replay (~40 elementwise kernels/step).  Keeping
            # the weights bf16 gives the IDENTICAL forward compute (autocast
            # rounds f32 weights to bf16 per use anyway) while the f32 master
            # copy preserves full-precision SGD accumulation — 4 multi-tensor
            # launches replace the per-layer cast storm.
            # PA_GRAPH_BF16=0 selects the autocast variant (A/B switch).
            # (model.bfloat16() itself ran before the DDP wrap, above)
            if bf16_weights and (world > 1 or bool(args.flat_params)):
                # SIDE-BAND flat scheme: every FusedLinear accumulates its
                # weight/bias gradient straight into ONE f32 flat buffer via
                # atomics inside wgrad/bias_grad (ops/dense.py _sideband) —
                # no per-layer dw materialization, f32->bf16 cast, pad-column
                # slice or AccumulateGrad add.  bf16 weights are views of an
                # aligned flat bf16 buffer with an f32 master; the f32 grad
                # buffer mirrors the weight layout so the SGD is one add +
                # one cast-copy.  Non-fused params (the 1-logit head) keep
                # preset bf16 grads, cast into their f32 slots per step.
                from persia_amd.ops.dense import FusedLinear

                fused_w, fused_b = [], []
                for m in model.modules():
                    if isinstance(m, FusedLinear):
                        fused_w.append(m.weight)
                        if isinstance(m.bias, torch.nn.Parameter):
                            fused_b.append(m.bias)
                fused_ids = {id(p) for p in fused_w + fused_b}
                other = [p for p in model.parameters() if id(p) not in fused_ids]
                bf_params = [p for p in model.parameters()
                             if p.dtype == torch.bfloat16]
                ALIGN = 128  # 256 B slots: misaligned views knock hipBLASLt
                # and the 16 B vector loads off their fast paths (measured)
                offs, off = {}, 0
                for p in bf_params:
                    off = (off + ALIGN - 1) // ALIGN * ALIGN
                    offs[id(p)] = off
                    off += p.numel()
                nw = off
                for p in fused_b + [q for q in other if q.dtype == torch.float32]:
                    off = (off + ALIGN - 1) // ALIGN * ALIGN
                    offs[id(p)] = off
                    off += p.numel()
                flat_w = torch.zeros(nw, dtype=torch.bfloat16, device=device)
                flat_g32 = torch.zeros(off, dtype=torch.float32, device=device)
                for p in bf_params:
                    o, n = offs[id(p)], p.numel()
                    flat_w[o : o + n].copy_(p.detach().view(-1))
                    with torch.no_grad():
                        p.data = flat_w[o : o + n].view_as(p)

                def gview(p):
                    return flat_g32[offs[id(p)] : offs[id(p)] + p.numel()].view_as(p)

                for p in fused_w + fused_b:
                    p._sideband_grad = gview(p)
                other_bf = [p for p in other if p.dtype == torch.bfloat16]
                other_f32 = [p for p in other if p.dtype == torch.float32]
                for p in other_bf + other_f32:
                    p.grad = torch.zeros_like(p)
                o_grads = [p.grad for p in other_bf + other_f32]
                o_views = [gview(p) for p in other_bf + other_f32]
                fb_views = [p._sideband_grad for p in fused_b]
                flat_master = flat_w.float()
                lr = opt.param_groups[0]["lr"]

                def sgd_body():
                    # allreduce (world>1) delivers the SUM: fold the 1/world
                    # average into the step
                    with torch.no_grad():
                        flat_master.add_(flat_g32[:nw], alpha=-lr / world)
                        flat_w.copy_(flat_master)
                        if fused_b:
                            torch._foreach_add_(fused_b, fb_views,
                                                alpha=-lr / world)
                        flat_g32.zero_()
                        if o_grads:
                            torch._foreach_zero_(o_grads)

                def iteration():
                    static["base"].grad.zero_()
                    logits = model(static["dense"], static["base"])
                    static["logits"] = logits.detach()  # no autograd graph kept alive
                    loss = loss_fn(logits.float(), static["label"])
                    loss.backward()
                    with torch.no_grad():
                        for gsrc, gdst in zip(o_grads, o_views):
                            gdst.copy_(gsrc)  # tiny head params
                    if world == 1:
                        sgd_body()
                    return loss

                if world > 1:
                    import torch.distributed as dist

                    # two-graph scheme: fwd+bwd graph, ONE f32 allreduce of
                    # the side-band flat gradients between the graphs, then
                    # the SGD graph (RCCL never captured)
                    flat_grads = flat_g32
                    update_body = sgd_body

                    def allreduce_grads():
                        dist.all_reduce(flat_g32)

            elif bf16_weights:
                # per-param foreach variant (PA_FLAT_PARAMS=0 A/B switch)
                g_params = list(model.parameters())
                g_masters = [p.detach().clone().float() for p in g_params]
                g_grads32 = [torch.zeros_like(m) for m in g_masters]
                lr = opt.param_groups[0]["lr"]
                for p in g_params:
                    p.grad = torch.zeros_like(p)

                def iteration():
                    static["base"].grad.zero_()
                    logits = model(static["dense"], static["base"])
                    static["logits"] = logits.detach()  # no autograd graph kept alive
                    loss = loss_fn(logits.float(), static["label"])
                    loss.backward()
                    grads = [p.grad for p in g_params]
                    torch._foreach_copy_(g_grads32, grads)
                    torch._foreach_add_(g_masters, g_grads32, alpha=-lr)
                    with torch.no_grad():
                        torch._foreach_copy_(g_params, g_masters)
                    torch._foreach_zero_(grads)
                    return loss

            else:

                def iteration():
                    static["base"].grad.zero_()
                    with torch.autocast("cuda", dtype=amp_dtype, cache_enabled=False):
                        logits = model(static["dense"], static["base"])
                        static["logits"] = logits.detach()  # no autograd graph kept alive
                        loss = loss_fn(logits.float(), static["label"])
                    loss.backward()
                    opt.step()
                    grads = [p.grad for p in model.parameters() if p.grad is not None]
                    torch._foreach_zero_(grads)
                    return loss

            # warmup on a side stream (allocator state, autotuned GEMMs)
            static["base"].grad = torch.zeros_like(static["base"], dtype=torch.float16)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(3):
                    iteration()
                    if flat_grads is not None:
                        allreduce_grads()
                        update_body()
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static["loss"] = iteration()
            if bf16_weights and world == 1 and "flat_w" in locals():
                # verify the captured backward writes the flat grad views
                # (a re-allocated .grad would silently train nothing): one
                # replay on random inputs must move the weights
                w0 = flat_w.float().sum().item()
                with torch.no_grad():
                    static["dense"].normal_()
                    static["base"].normal_()
                graph.replay()
                torch.cuda.synchronize()
                if flat_w.float().sum().item() == w0:
                    raise RuntimeError("flat-param capture trained nothing")
                with torch.no_grad():
                    static["dense"].zero_()
                    static["base"].zero_()
            if flat_grads is not None:
                # verify the captured backward really accumulates into the
                # flat views (autograd may re-allocate .grad instead of
                # adding in place, which would silently train nothing)
                with torch.no_grad():
                    static["dense"].normal_()
                    static["base"].normal_()
                graph.replay()
                torch.cuda.synchronize()
                if float(flat_grads.float().abs().sum().item()) == 0.0:
                    raise RuntimeError("flat-grad capture yielded no gradients")
                with torch.no_grad():
                    static["dense"].zero_()
                    static["base"].zero_()
                graph_upd = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph_upd):
                    update_body()
        except Exception as e:  # pragma: no cover - fall back to eager
            import sys as _sys

            print(f"# hipGraph capture failed ({e}); running eager",
                  file=_sys.stderr, flush=True)
            graph = None
            graph_upd = None
            for p in model.parameters():  # sideband only valid under the graph
                if hasattr(p, "_sideband_grad"):
                    del p._sideband_grad
            if world > 1 and defer_ddp:
                # the eager fallback still needs synchronized dense grads
                for p in model.parameters():
                    p.grad = None
                model = _wrap_ddp(model)
                opt = torch.optim.SGD(model.parameters(), lr=0.01)

    timing = os.environ.get("PA_BENCH_TIMING", "0") == "1"
    tstats = {"get": 0.0, "copy": 0.0, "replay": 0.0, "apply": 0.0, "n": 0}

    # Overlapped sparse update (PA_OVERLAP_UPDATE=1 enables; default OFF —
    # measured NEGATIVE): the fused table update runs on a dedicated stream
    # from a STAGED copy of the base gradient so the main stream serializes
    # only on the stage copy.  A/B on a fresh box: criteo 6.71M overlapped
    # vs 6.80M serial (the step is bound by the LOOKUP stream, so hiding
    # main-stream work buys nothing) and dcn-spill 1.73M vs ~3.4M (the
    # side-stream update steals HBM bandwidth from the sparse-critical
    # producer).  Kept as a gated experiment; ordering stays safe (updates
    # serialized on one stream; eviction-vs-update races are the same
    # bounded-staleness noise as the base design, csrc/kernels.hip notes).
    upd_stream = None
    if graph is not None and os.environ.get("PA_OVERLAP_UPDATE", "0") == "1":
        upd_stream = torch.cuda.Stream()
        upd_gstage = torch.zeros_like(static["base"].grad)
        ev_bwd = torch.cuda.Event()
        ev_staged = torch.cuda.Event()

    last = {}  # what the most recent eager step produced (--dump-outputs)

    def train_step(tb):
        if graph is not None:
            if timing:
                t0 = time.perf_counter()
            with torch.no_grad():
                static["dense"][:, : args.num_dense].copy_(
                    tb.non_id_type_tensors[0], non_blocking=True
                )
                static["base"].copy_(tb._groups[0].sum_base, non_blocking=True)
                static["label"].copy_(tb.label_tensors[0], non_blocking=True)
            if timing:
                t1 = time.perf_counter()
            graph.replay()
            if upd_stream is not None:
                ev_bwd.record()
                upd_stream.wait_event(ev_bwd)
                with torch.cuda.stream(upd_stream):
                    upd_gstage.copy_(static["base"].grad, non_blocking=True)
                    ev_staged.record(upd_stream)
                    engine.apply_gradients_base(tb, sum_base_grads=[upd_gstage])
                    tb.record_stream(upd_stream)
            if graph_upd is not None:
                allreduce_grads()
                graph_upd.replay()
            if timing:
                t2 = time.perf_counter()
            if upd_stream is not None:
                # gate the next replay (which zeroes base.grad) on the stage
                # copy only — the table update continues on upd_stream
                torch.cuda.current_stream().wait_event(ev_staged)
            else:
                engine.apply_gradients_base(
                    tb, sum_base_grads=[static["base"].grad]
                )
            pipeline.release_permit()
            if timing:
                t3 = time.perf_counter()
                tstats["copy"] += t1 - t0
                tstats["replay"] += t2 - t1
                tstats["apply"] += t3 - t2
                tstats["n"] += 1
            return static["loss"]
        with amp_ctx:
            embs = tb.training_embeddings()
            logits = model(tb.non_id_type_tensors, embs)
            loss = loss_fn(logits.float(), tb.label_tensors[0])
        last["logits"], last["loss"] = logits.detach(), loss.detach()
        loss.backward()
        engine.apply_gradients_base(tb)
        opt.step()
        opt.zero_grad(set_to_none=True)
        pipeline.release_permit()
        return loss

    import threading

    def feed(start, n):
        for i in range(start, start + n):
            pipeline.put(host_batches[i % len(host_batches)])

    # warmup: feed + consume, then drain so NO timed batch has its sparse work
    # pre-done before t0 (the staleness window only overlaps WITHIN the timed
    # region — keeps the measurement honest for any step count).  Warmup
    # covers at least one full pass over the host-batch pool so the working
    # set is table-resident and the timed region measures the hit
    # steady-state (matching long-soak numbers) instead of the one-time
    # insert transient; the JSON reports the warmup actually executed.
    warm_steps = max(args.warmup, len(host_batches) + 2)
    threading.Thread(target=feed, args=(0, warm_steps), daemon=True).start()
    for _ in range(warm_steps):
        train_step(pipeline.get())

    if world > 1:
        import torch.distributed as dist

        dist.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    feeder = threading.Thread(target=feed, args=(warm_steps, args.steps), daemon=True)
    feeder.start()
    for _ in range(args.steps):
        tg0 = time.perf_counter() if timing else 0.0
        tb = pipeline.get()
        if timing:
            tstats["get"] += time.perf_counter() - tg0
        train_step(tb)
    if world > 1:
        dist.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device if use_gpu else None)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    pipeline.stop()
    if args.dump_outputs and rank == 0:
        if graph is not None:
            out, base = static, static["base"]
        else:
            out, base = last, tb._groups[0].sum_base
        _dump_outputs(
            args.dump_outputs,
            loss=out["loss"],
            logits=out["logits"],
            dense_params=torch.cat(
                [p.detach().reshape(-1).float() for p in model.parameters()]
            ),
            emb_sum=base,
            emb_sum_grad=None if base is None else base.grad,
        )
    if world > 1:
        # the padded-a2a fast path drops keys to a dummy slot on bucket
        # overflow (probability ~exp(-20 sigma) with the default slack);
        # surface it loudly if the heuristic ever failed
        ovf = engine.check_a2a_overflow()
        if ovf:
            import sys as _sy

            print(f"# WARNING: padded-a2a bucket overflow on {ovf} batches "
                  f"(keys dropped; widen the cap slack)",
                  file=_sy.stderr, flush=True)
    if timing and tstats["n"]:
        import sys as _s

        n = tstats["n"]
        prod = (
            pipeline.prod_s / pipeline.prod_n * 1e3 if pipeline.prod_n else 0.0
        )
        print(
            f"# phase ms/step: get={tstats['get']/n*1e3:.3f} "
            f"copy={tstats['copy']/n*1e3:.3f} replay={tstats['replay']/n*1e3:.3f} "
            f"apply={tstats['apply']/n*1e3:.3f} producer={prod:.3f}",
            file=_s.stderr, flush=True,
        )
        pt = engine._pt
        if pt["n"]:
            pn = pt["n"]
            extra = "".join(
                f" {k}={pt[k]/pn*1e3:.3f}"
                for k in ("dedup", "exch", "route", "lkw", "sum") if k in pt
            )
            print(
                f"# producer ms/batch: total={pt['batch']/pn*1e3:.3f} "
                f"prep={pt['prep']/pn*1e3:.3f} native={pt['native']/pn*1e3:.3f}"
                + extra,
                file=_s.stderr, flush=True,
            )
    samples = args.steps * B * world
    if rank == 0:
        result = {
            "metric": "samples/sec (whole node), DLRM-style hybrid training",
            "value": samples / elapsed,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": warm_steps,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic (uniform ids, random labels, random-init weights)",
            "config": {
                "preset": args.preset,
                "model": f"{args.model} {args.num_sparse}sparse/{args.num_dense}dense dim{dim}",
                "global_batch": B * world,
                "rows": rows_total,
                "capacity_per_rank": capacity,
                "staleness": args.staleness,
                "parallelism": f"dp{world}+emb-a2a",
            },
        }
        print(json.dumps(result))
    if world > 1:
        dist.destroy_process_group()


DUMP_MAX_ELEMS = 1 << 21  # per array: 8 MB of float32, 5 arrays < 64 MB


def _dump_outputs(dst, **arrays):
    """Write each array as dst/<name>.npy in float32.  An array larger than
    DUMP_MAX_ELEMS is reduced to a fixed sample of its flattened elements
    (seeded by its size only, so two builds pick the same elements)."""
    os.makedirs(dst, exist_ok=True)
    for name, t in arrays.items():
        if t is None:
            continue
        flat = t.detach().reshape(-1)
        if flat.numel() > DUMP_MAX_ELEMS:
            idx = np.sort(
                np.random.default_rng(flat.numel()).integers(
                    0, flat.numel(), size=DUMP_MAX_ELEMS
                )
            )
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        np.save(os.path.join(dst, name + ".npy"), flat.float().cpu().numpy())


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


if __name__ == "__main__":
    main()
