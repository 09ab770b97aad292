"""End-to-end GPU training smoke + learning test (MI355X box)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_dlrm_train_loop_learns():
    from persia_amd.core.comm import DistContext
    from persia_amd.core.engine import EmbeddingEngine, ForwardPipeline
    from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
    from persia_amd.embedding import EmbeddingConfig
    from persia_amd.embedding.data import IDTypeFeatureWithSingleID, Label, PersiaBatch
    from persia_amd.embedding.optim import Adagrad
    from persia_amd.models import DLRM

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    n_slots, dim, B, vocab = 8, 32, 256, 1000
    schema = EmbeddingSchema(
        slots={f"f{i}": SlotConfig(name=f"f{i}", dim=dim) for i in range(n_slots)}
    )
    engine = EmbeddingEngine(
        schema=schema,
        hyper=EmbeddingConfig(),
        optimizer=Adagrad(lr=0.05),
        gconf=GlobalConfig(capacity=1 << 18),
        device=device,
        dist_ctx=DistContext(1, 0),
    )
    model = DLRM(num_sparse=n_slots, num_dense=4, dim=dim).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)

    rng = np.random.default_rng(0)
    id_scores = rng.normal(size=vocab)

    def mk_batch():
        ids = rng.integers(0, vocab, size=(B, n_slots), dtype=np.uint64)
        label = (id_scores[ids].sum(axis=1) > 0).astype(np.float32)
        dense = rng.normal(size=(B, 4)).astype(np.float32)
        feats = [
            IDTypeFeatureWithSingleID(f"f{i}", ids[:, i].copy()) for i in range(n_slots)
        ]
        return PersiaBatch(
            feats, non_id_type_features=[dense], labels=[Label(label)], requires_grad=True
        )

    pipeline = ForwardPipeline(engine, staleness=2)
    pipeline.start()
    n_steps = 250
    batches = [mk_batch() for _ in range(10)]
    import threading

    def feed():
        for i in range(n_steps):
            pipeline.put(batches[i % len(batches)])

    threading.Thread(target=feed, daemon=True).start()

    losses = []
    for _ in range(n_steps):
        tb = pipeline.get(timeout=120)
        embs = tb.training_embeddings()
        logits = model(tb.non_id_type_tensors, embs)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(
            logits.float(), tb.label_tensors[0]
        )
        loss.backward()
        engine.apply_gradients_base(tb)
        opt.step()
        opt.zero_grad(set_to_none=True)
        pipeline.release_permit()
        losses.append(float(loss.detach()))
    pipeline.stop()
    assert all(np.isfinite(losses))
    assert np.mean(losses[-20:]) < np.mean(losses[:20]) - 0.02, (
        losses[:20], losses[-20:]
    )
    assert engine.num_resident_rows() > 0


def test_adult_income_gpu_deterministic():
    """The reference's GPU correctness anchor (train.py:24 GPU_TEST_AUC):
    deterministic mode reproduces bitwise on the GPU engine too."""
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run_once():
        env = dict(os.environ)
        env.update(REPRODUCIBLE="1", EMBEDDING_STALENESS="1")
        code = (
            "import sys; sys.path.insert(0, r'%s'); sys.path.insert(0, r'%s');"
            "import train; a, b = train.main(epochs=1); print('AUCS', repr(a), repr(b))"
            % (os.path.join(repo, "examples", "adult_income"), repo)
        )
        out = subprocess.run(
            [sys.executable, "-c", code],
            cwd=os.path.join(repo, "examples", "adult_income"),
            env=env, capture_output=True, text=True, timeout=900,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        return [l for l in out.stdout.splitlines() if l.startswith("AUCS")][0]

    a1 = run_once()
    a2 = run_once()
    assert a1 == a2, f"GPU deterministic mode must reproduce: {a1} != {a2}"
    train_repr = a1.split()[1].split("(")[-1].rstrip(")")
    # pinned golden constant (analog of reference GPU_TEST_AUC, train.py:24):
    # captured 2026-09-14, 1 MI355X, REPRODUCIBLE=1, staleness=1
    assert train_repr == GPU_TRAIN_AUC, (
        f"GPU train AUC drifted from the golden constant: {train_repr} != "
        f"{GPU_TRAIN_AUC} — a cross-commit numerics regression"
    )


GPU_TRAIN_AUC = "0.8791397180312086"  # captured 2026-09-14 on MI355X


def test_bench_default_config_one_step(tmp_path):
    """bench.py's engine wiring at the flagship shape (tiny step count); the
    graphed path also dumps its last step's outputs."""
    import subprocess
    import sys
    import json
    import os

    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1",
         "--batch-size", "1024", "--rows", "1e6",
         "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=600,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["value"] > 0
    assert res["n_gpus"] == 1
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    names = set(os.listdir(tmp_path))
    assert names == {"loss.npy", "logits.npy", "dense_params.npy",
                     "emb_sum.npy", "emb_sum_grad.npy"}, names
    total = 0
    for n in names:
        a = np.load(os.path.join(tmp_path, n))
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 * 1000 * 1000
    assert np.load(os.path.join(tmp_path, "logits.npy")).size == 1024
    assert np.abs(np.load(os.path.join(tmp_path, "emb_sum_grad.npy"))).max() > 0


def test_flat_grad_views_accumulate_inside_graph():
    """bench.py's multi-GPU graph mode points every param.grad at a view of
    ONE flat bf16 buffer and captures fwd+bwd; autograd must accumulate into
    those views IN PLACE (a silent re-allocation would train nothing)."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    model = torch.nn.Sequential(
        torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 1)
    ).to(dev).bfloat16()
    params = list(model.parameters())
    flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.bfloat16, device=dev)
    off = 0
    for p in params:
        p.grad = flat[off : off + p.numel()].view_as(p)
        off += p.numel()
    x = torch.randn(64, 16, device=dev, dtype=torch.bfloat16)
    y = torch.randn(64, device=dev, dtype=torch.bfloat16)

    def iteration():
        torch._foreach_zero_([flat])
        loss = ((model(x).squeeze(1) - y) ** 2).mean()
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            iteration()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        iteration()
    g.replay()
    torch.cuda.synchronize()
    total = float(flat.float().abs().sum().item())
    assert total > 0.0, "captured backward did not write the flat grad views"
    # the python-side .grad objects must still BE the views
    assert params[0].grad.data_ptr() == flat.data_ptr()
