"""End-to-end single-process CPU training: the reference adult-income-style
correctness anchor (deterministic mode reproduces bitwise-identical results;
the model actually learns a separable synthetic task)."""
import numpy as np
import torch

from persia_amd.ctx import TrainCtx, eval_ctx
from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
from persia_amd.data import DataLoader, IterableDataset
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.data import IDTypeFeature, Label, NonIDTypeFeature, PersiaBatch
from persia_amd.embedding.optim import Adagrad
from persia_amd.models import CTRModel
from persia_amd.utils import setup_seed


N_SLOTS = 4
DIM = 16
VOCAB = 50


def _schema():
    return EmbeddingSchema(
        slots={f"s{i}": SlotConfig(name=f"s{i}", dim=DIM) for i in range(N_SLOTS)},
    )


class SynthDataset(IterableDataset):
    """Labels depend on the sparse ids -> learnable only through embeddings."""

    def __init__(self, n_batches=30, batch_size=32, seed=0, requires_grad=True, epochs=1):
        super().__init__(buffer_size=10)
        self.n_batches = n_batches
        self.batch_size = batch_size
        self.seed = seed
        self.requires_grad = requires_grad
        self.epochs = epochs

    def __iter__(self):
        rng = np.random.default_rng(self.seed)
        # per-id score table -> labels linearly separable through embeddings
        id_scores = rng.normal(size=VOCAB)
        batches = []
        for _ in range(self.n_batches):
            ids = rng.integers(0, VOCAB, size=(self.batch_size, N_SLOTS), dtype=np.uint64)
            label = (id_scores[ids].sum(axis=1) > 0).astype(np.float32).reshape(-1, 1)
            dense = rng.normal(size=(self.batch_size, 5)).astype(np.float32)
            batches.append((ids, label, dense))
        for _ in range(self.epochs):
            for ids, label, dense in batches:
                yield self._make(ids, label, dense)

    def _make(self, ids, label, dense):
        feats = [
            IDTypeFeature(f"s{i}", [ids[b, i : i + 1] for b in range(self.batch_size)])
            for i in range(N_SLOTS)
        ]
        return PersiaBatch(
            feats,
            non_id_type_features=[NonIDTypeFeature(dense)],
            labels=[Label(label)],
            requires_grad=self.requires_grad,
        )


def _train_once(seed=3, n_batches=40):
    setup_seed(seed)
    model = CTRModel(num_dense=5, sparse_input_dim=N_SLOTS * DIM)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    losses = []
    with TrainCtx(
        model=model,
        embedding_optimizer=Adagrad(lr=0.05),
        dense_optimizer=opt,
        embedding_config=EmbeddingConfig(),
        embedding_schema=_schema(),
        global_config=GlobalConfig(capacity=1 << 14),
        mixed_precision=False,
        device_id=-1,
    ) as ctx:
        loader = DataLoader(
            SynthDataset(n_batches=n_batches // 4, batch_size=64, epochs=4),
            reproducible=True,
            embedding_staleness=1,
        )
        loss_fn = torch.nn.BCELoss()
        for tb in loader:
            pred, labels = ctx.forward(tb)
            loss = loss_fn(pred.squeeze(1), labels[0].squeeze(1))
            ctx.backward(loss)
            losses.append(float(loss.detach()))
    return losses, model


def test_training_learns_and_is_deterministic():
    losses1, _ = _train_once()
    losses2, _ = _train_once()
    # deterministic mode: bitwise-identical loss trajectory
    assert losses1 == losses2
    # learning: last-quarter mean loss clearly below first-quarter
    q = len(losses1) // 4
    assert np.mean(losses1[-q:]) < np.mean(losses1[:q]) - 0.05


def test_eval_ctx_shares_engine():
    losses, model = _train_once(n_batches=10)
    model.eval()
    # same device as the TrainCtx whose engine it shares (a bare eval_ctx
    # would pick cuda:0 on a GPU machine and move the model off the engine)
    with eval_ctx(model=model, device_id=-1) as ctx:
        for tb in DataLoader(SynthDataset(n_batches=2, requires_grad=False)):
            pred, labels = ctx.forward(tb)
            assert pred.shape[0] == 32
            assert labels is not None
    model.train()


def test_ctx_checkpoint_roundtrip(tmp_path):
    """User-facing full checkpoint (reference ctx.py:471-652): dump dense
    state dict + embedding shards, reload into a FRESH ctx, and verify both
    the dense parameters and the embedding outputs survive exactly."""
    def make_ctx(seed):
        setup_seed(seed)
        model = CTRModel(num_dense=5, sparse_input_dim=N_SLOTS * DIM)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        return TrainCtx(
            model=model,
            dense_optimizer=opt,
            embedding_optimizer=Adagrad(lr=0.1),
            embedding_config=EmbeddingConfig(),
            embedding_schema=_schema(),
            global_config=GlobalConfig(capacity=1 << 14),
            mixed_precision=False,
            device_id=-1,
        )

    ctx = make_ctx(7)
    loader = DataLoader(SynthDataset(n_batches=6, batch_size=16, seed=3), embedding_staleness=2)
    loss_fn = torch.nn.BCELoss()
    with ctx:
        for tb in loader:
            pred, labels = ctx.forward(tb)
            loss = loss_fn(pred.squeeze(1), labels[0].squeeze(1))
            ctx.backward(loss)
        ctx.dump_checkpoint(str(tmp_path))
        sizes = ctx.get_embedding_size()
        assert sizes and sizes[0] > 0
        # capture a reference forward AFTER training
        probe = SynthDataset(n_batches=1, batch_size=16, seed=9, requires_grad=False)
        batch = next(iter(probe))
        ref_tb = ctx.engine.process_batch(batch, train=False)
        ref_out = [p.sum_tensor.clone() for p in ref_tb.payloads]
        ref_state = {
            k: v.clone() for k, v in ctx.model.state_dict().items()
        }

    ctx2 = make_ctx(8)  # different seed: different init before load
    with ctx2:
        ctx2.load_checkpoint(str(tmp_path))
        for k, v in ctx2.model.state_dict().items():
            assert torch.equal(v, ref_state[k]), k
        tb2 = ctx2.engine.process_batch(
            next(iter(SynthDataset(n_batches=1, batch_size=16, seed=9,
                                   requires_grad=False))),
            train=False,
        )
        for a, b in zip(ref_out, tb2.payloads):
            assert torch.equal(a, b.sum_tensor)
        # clear_embeddings drops every resident row
        ctx2.clear_embeddings()
        assert sum(ctx2.get_embedding_size()) == 0
