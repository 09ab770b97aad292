"""Pins of the engine's lookup/update paths: the two update contracts agree,
a skipped group or slot leaves no trace, and (tests/test_gpu_engine_paths.py,
which reuses the helpers here) the GPU paths agree with the CPU engine and
with each other.

Shapes: B=32, dims 8 and 16, vocabulary 300, capacity 1<<14 (no eviction),
3 steps.
"""
import numpy as np
import pytest
import torch

from persia_amd.core.comm import DistContext
from persia_amd.core.engine import EmbeddingEngine
from persia_amd.core.schema import (
    EmbeddingSchema, GlobalConfig, HashStackConfig, SlotConfig,
)
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.data import (
    IDTypeFeature, IDTypeFeatureWithSingleID, Label, PersiaBatch,
)
from persia_amd.embedding.optim import Adagrad, Adam

B = 32
VOCAB = 300
STEPS = 3
CPU = torch.device("cpu")
SINGLE_SLOTS = {"a": 8, "b": 8, "c": 16, "d": 16}  # name -> dim


def mk_opt(name):
    return Adam(lr=0.01) if name == "adam" else Adagrad(lr=0.1)


def single_schema():
    return EmbeddingSchema(
        slots={n: SlotConfig(name=n, dim=d) for n, d in SINGLE_SLOTS.items()}
    )


def mixed_schema():
    """The slot mix of test_engine_gpu_matches_cpu_engine (sum, sum+sqrt,
    raw with sample_fixed_size, hashstack) plus a dim-8 sum slot."""
    return EmbeddingSchema(
        slots={
            "a": SlotConfig(name="a", dim=16),
            "b": SlotConfig(name="b", dim=16, sqrt_scaling=True),
            "r": SlotConfig(name="r", dim=16, embedding_summation=False,
                            sample_fixed_size=4),
            "h": SlotConfig(
                name="h", dim=16,
                hash_stack_config=HashStackConfig(
                    hash_stack_rounds=2, embedding_size=64
                ),
            ),
            "e": SlotConfig(name="e", dim=8),
        }
    )


def mk_engine(device, optname, schema=None, **gconf):
    gconf.setdefault("capacity", 1 << 14)
    return EmbeddingEngine(
        schema=schema or single_schema(),
        hyper=EmbeddingConfig(emb_initialization=(-0.5, 0.5)),
        optimizer=mk_opt(optname),
        gconf=GlobalConfig(**gconf),
        device=device,
        dist_ctx=DistContext(1, 0),
    )


def single_batch(seed, names=tuple(SINGLE_SLOTS), batch_size=B):
    rng = np.random.default_rng(seed)
    feats = [
        IDTypeFeatureWithSingleID(
            n, rng.integers(0, VOCAB, size=batch_size, dtype=np.uint64)
        )
        for n in names
    ]
    return PersiaBatch(
        feats, labels=[Label(np.ones((batch_size, 1), np.float32))],
        requires_grad=True,
    )


def list_batch(seed):
    """single_batch's ids as one-element lists: the same lookups through the
    generic (variable-length) path instead of the all-single-ID fast path."""
    single = single_batch(seed)
    feats = [
        IDTypeFeature(f.name, [np.array([v], dtype=np.uint64) for v in f.values])
        for f in single.id_type_features
    ]
    return PersiaBatch(feats, labels=[Label(np.ones((B, 1), np.float32))],
                       requires_grad=True)


def mixed_batch(seed):
    """Variable lengths 0..5 per sample: empty samples included."""
    rng = np.random.default_rng(seed)
    feats = [
        IDTypeFeature(
            n, [rng.integers(0, VOCAB, size=rng.integers(0, 6), dtype=np.uint64)
                for _ in range(B)]
        )
        for n in ("a", "b", "r", "h", "e")
    ]
    return PersiaBatch(feats, labels=[Label(np.ones((B, 1), np.float32))],
                       requires_grad=True)


def slot_grads(seed, device, names=tuple(SINGLE_SLOTS)):
    """Seeded (B, dim) f16 gradient per single-ID sum slot."""
    gen = torch.Generator().manual_seed(seed)
    return {
        n: torch.randn(B, SINGLE_SLOTS[n], generator=gen).half().to(device)
        for n in names
    }


def set_base_grads(tb, grads):
    """Place per-slot gradients into each group's ``sum_base.grad`` (what
    autograd leaves there after ``enable_training_views``)."""
    for group in tb._groups:
        group.sum_base.requires_grad_(True)
        group.sum_base.grad = torch.cat(
            [grads[sc.name] for sc in group.slots if sc.cfg.embedding_summation]
        )


def table(engine):
    """dim -> (signs ascending, rows in that order) of every store."""
    if engine.device.type == "cuda":
        torch.cuda.synchronize()
    out = {}
    for dim, store in engine.stores.items():
        signs, rows = store.export_rows()
        order = np.argsort(signs)
        out[dim] = (signs[order], rows[order])
    return out


def assert_tables_equal(t1, t2):
    assert t1.keys() == t2.keys()
    for dim in t1:
        assert np.array_equal(t1[dim][0], t2[dim][0]), f"dim {dim}: signs"
        assert np.array_equal(t1[dim][1], t2[dim][1]), f"dim {dim}: rows"


def tables_differ(t1, t2):
    return any(not np.array_equal(t1[d][1], t2[d][1]) for d in t1)


def lookups_only(device, optname):
    """The table after the STEPS single-ID lookups and no update."""
    eng = mk_engine(device, optname)
    for step in range(STEPS):
        eng.process_batch(single_batch(step))
    return table(eng)


# ------------------------------------------------ 1. the two update contracts


@pytest.mark.parametrize("loss_scale", [1.0, 4.0])
@pytest.mark.parametrize("optname", ["adagrad", "adam"])
def test_update_contracts_agree_bitwise_cpu(optname, loss_scale):
    """apply_gradients (per-slot dict) and apply_gradients_base (the same
    values in sum_base.grad) leave bit-identical tables; with Adam that also
    pins one beta-power step per update call."""
    eng_dict = mk_engine(CPU, optname)
    eng_base = mk_engine(CPU, optname)
    for step in range(STEPS):
        grads = slot_grads(100 + step, CPU)
        tb = eng_dict.process_batch(single_batch(step))
        eng_dict.apply_gradients(tb, grads, loss_scale=loss_scale)
        tb = eng_base.process_batch(single_batch(step))
        set_base_grads(tb, grads)
        eng_base.apply_gradients_base(tb, loss_scale=loss_scale)
    assert tables_differ(lookups_only(CPU, optname), table(eng_dict))
    assert_tables_equal(table(eng_dict), table(eng_base))


def test_update_counter_advances_once_per_call_cpu():
    """Both entry points advance the sampling counter once per call — also on
    CPU, where the base contract runs through the per-slot one."""
    eng = mk_engine(CPU, "adagrad")
    tb = eng.process_batch(single_batch(0))
    eng.apply_gradients(tb, slot_grads(100, CPU))
    assert eng._update_counter == 1
    tb = eng.process_batch(single_batch(1))
    set_base_grads(tb, slot_grads(101, CPU))
    eng.apply_gradients_base(tb)
    assert eng._update_counter == 2


# ---------------------------------------------------------- 3. skip semantics


def check_skipped_group_leaves_no_trace(device, contract, mk_batch=single_batch):
    """A group with no gradient at all is skipped: the table stays
    bit-identical, and (Adam) the beta powers do not move — the next real
    update matches an engine that never saw the skipped batch.  The skipped
    batch repeats step 0's ids, so its lookups insert nothing."""
    seen = mk_engine(device, "adam")
    never = mk_engine(device, "adam")

    def real_step(eng, step):
        tb = eng.process_batch(mk_batch(step))
        set_base_grads(tb, slot_grads(100 + step, device))
        eng.apply_gradients_base(tb)

    real_step(seen, 0)
    real_step(never, 0)
    before = table(seen)
    tb = seen.process_batch(mk_batch(0))
    if contract == "dict":
        seen.apply_gradients(tb, {n: None for n in SINGLE_SLOTS})
    else:
        assert all(g.sum_base.grad is None for g in tb._groups)
        seen.apply_gradients_base(tb)
    assert_tables_equal(before, table(seen))
    real_step(seen, 1)
    real_step(never, 1)
    assert tables_differ(before, table(seen))
    assert_tables_equal(table(seen), table(never))


def check_nan_slot_is_dropped_alone(device, mk_batch=single_batch):
    """Dict contract: a NaN in one slot's gradient zeroes that slot's
    contribution only — the result equals a run where that slot's gradient
    was None, and the other slots' rows did move."""
    eng_nan = mk_engine(device, "adagrad")
    eng_none = mk_engine(device, "adagrad")
    for step in range(STEPS):
        grads = slot_grads(100 + step, device)
        bad = dict(grads)
        bad["a"] = grads["a"].clone()
        bad["a"][3, 1] = float("nan")
        dropped = dict(grads, a=None)
        eng_nan.apply_gradients(eng_nan.process_batch(mk_batch(step)), bad)
        eng_none.apply_gradients(eng_none.process_batch(mk_batch(step)), dropped)
    assert_tables_equal(table(eng_nan), table(eng_none))
    # slot b shares dim-group 8 with the NaN slot: its rows were trained
    untrained, trained = lookups_only(device, "adagrad"), table(eng_nan)
    assert tables_differ({8: untrained[8]}, {8: trained[8]})
    return eng_nan


@pytest.mark.parametrize("contract", ["dict", "base"])
def test_skipped_group_leaves_no_trace_cpu(contract):
    check_skipped_group_leaves_no_trace(CPU, contract)


def test_nan_slot_is_dropped_alone_cpu():
    eng = check_nan_slot_is_dropped_alone(CPU)
    assert eng.nan_grad_batches == STEPS
