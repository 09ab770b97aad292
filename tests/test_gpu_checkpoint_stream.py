"""Streaming checkpoint on the HIP backend (csrc/checkpoint.hip):
export_chunks / import_chunk against the whole-table export_rows /
import_rows, bit for bit, plus the bounded-memory guarantee and the engine
end to end."""
import filecmp
import os

import numpy as np
import pytest
import torch

from persia_amd.core import hashing
from persia_amd.core.comm import DistContext
from persia_amd.core.store import _adapt_row_width

pytestmark = pytest.mark.gpu

N_ROWS = 1500
ZERO_REMAP = 0xD1B54A32D192ED03


def _dev():
    return torch.device("cuda", 0)


def _signs():
    return np.random.default_rng(1234).integers(1, 2 ** 63, size=N_ROWS, dtype=np.uint64)


def _rows(width, seed=99):
    return np.random.default_rng(seed).standard_normal((N_ROWS, width)).astype(np.float32)


def _optim(name):
    from persia_amd.embedding.optim import SGD, Adagrad, Adam

    return {
        "sgd": lambda: SGD(lr=0.1),
        "adagrad": lambda: Adagrad(lr=0.1, initial_accumulator_value=0.01),
        "adagrad_shared": lambda: Adagrad(lr=0.1, vectorwise_shared=True),
        "adam": lambda: Adam(lr=0.01),
    }[name]()


def _store(optim, dim=8, capacity=4096, spill_capacity=0):
    from persia_amd.core.store import HipEmbeddingStore
    from persia_amd.embedding import EmbeddingConfig

    return HipEmbeddingStore(
        dim=dim, capacity=capacity, optimizer=_optim(optim),
        hyper=EmbeddingConfig(), device=_dev(), spill_capacity=spill_capacity,
    )


def _mix(signs):
    return torch.from_numpy(hashing.splitmix64(signs).view(np.int64)).to(_dev())


def _collect(store, chunk_rows):
    """Concatenated copy of a full export_chunks pass (pieces are only valid
    until the generator is advanced)."""
    parts = [(s.copy(), i.copy()) for s, i in store.export_chunks(chunk_rows)]
    assert all(0 < len(s) <= chunk_rows and len(s) == len(i) for s, i in parts)
    if not parts:
        return (np.zeros(0, np.uint64),
                np.zeros((0, store.row_width), np.float32))
    return (np.concatenate([s for s, _ in parts]),
            np.concatenate([i for _, i in parts]))


def _assert_same_export(store, chunk_rows):
    want_s, want_i = store.export_rows()
    got_s, got_i = _collect(store, chunk_rows)
    assert got_s.dtype == np.uint64 and got_i.dtype == np.float32
    assert got_i.shape == want_i.shape
    assert np.array_equal(got_s, want_s)
    assert np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32))
    return want_s


def _sorted(signs, inner):
    o = np.argsort(signs)
    return signs[o], inner[o].view(np.uint32)


# ------------------------------------------------------------------- export


@pytest.mark.parametrize(
    "optim,dim,width",
    [("sgd", 8, 8), ("adagrad", 8, 16), ("adagrad_shared", 8, 9), ("adam", 8, 24),
     ("adagrad", 128, 256)],
)
def test_export_chunks_equal_export_rows(optim, dim, width):
    store = _store(optim, dim=dim)
    assert store.row_width == width and store.n_slots == 4096
    keys = _mix(_signs())
    store.lookup(keys, train=True)
    g = torch.Generator(device="cpu").manual_seed(5)
    store.update_gradients(keys, torch.randn(N_ROWS, dim, generator=g).to(_dev()))
    for c in (64, 1000, 4096, 10000):
        signs = _assert_same_export(store, c)
    assert len(signs) > 1400  # the table really holds the rows


def _craft(store, occupied, seed=3):
    """Write keys and arena directly: export does not probe, so any
    placement is legal."""
    rng = np.random.default_rng(seed)
    keys = np.zeros(store.n_slots, dtype=np.uint64)
    keys[occupied] = rng.integers(1, 2 ** 64 - 1, size=len(occupied), dtype=np.uint64)
    store.keys.copy_(torch.from_numpy(keys.view(np.int64)))
    store.arena.copy_(
        torch.from_numpy(
            rng.standard_normal((store.n_slots, store.row_width)).astype(np.float32)
        )
    )
    return keys


@pytest.mark.parametrize("optim,width", [("sgd", 8), ("adagrad_shared", 9)])
def test_export_crafted_occupancy(optim, width):
    store = _store(optim)
    W, n = 64, store.n_slots
    full_w, empty_w = 5, 9
    occ = {0, n - 1}
    for b in range(W, n, W):  # both sides of every window boundary
        occ.update((b - 1, b))
    occ.update(range(full_w * W, (full_w + 1) * W))  # one completely full window
    occ.update((100, 101, 777, 1023, 1024, 1025, 2047, 2048, 3000))
    occ -= set(range(empty_w * W, (empty_w + 1) * W))  # one completely empty
    occ = np.array(sorted(occ), dtype=np.int64)
    keys = _craft(store, occ)
    for c in (64, 1000, 4096):
        signs = _assert_same_export(store, c)
    # ascending slot order, signs un-mixed on the device
    assert np.array_equal(signs, hashing.splitmix64_inv(keys[occ]))


def test_export_every_slot_occupied():
    store = _store("sgd")
    _craft(store, np.arange(store.n_slots))
    for c in (64, 1000):
        assert len(_assert_same_export(store, c)) == store.n_slots


def test_export_empty_store():
    store = _store("adagrad")
    assert list(store.export_chunks(64)) == []
    assert len(_assert_same_export(store, 64)) == 0


def test_export_zero_remap_key():
    store = _store("sgd")
    sign0 = hashing.splitmix64_inv(np.zeros(1, dtype=np.uint64))
    signs = np.concatenate([sign0, np.arange(1, 40, dtype=np.uint64)])
    inner = _rows(8)[:40]
    store.import_chunk(signs, inner)
    assert store.finish_import() == 0
    remap_i64 = int(np.array([ZERO_REMAP], dtype=np.uint64).view(np.int64)[0])
    assert int((store.keys == remap_i64).sum().item()) == 1
    # neither path un-remaps: both report splitmix64_inv(remap key)
    got = _assert_same_export(store, 64)
    assert len(got) == 40
    remapped = hashing.splitmix64_inv(np.array([ZERO_REMAP], dtype=np.uint64))[0]
    assert remapped in got and sign0[0] not in got


# ------------------------------------------------------------------- import


@pytest.mark.parametrize(
    "optim,dim,width",
    [("sgd", 8, 8), ("adagrad_shared", 8, 9), ("adagrad", 8, 16), ("adagrad", 128, 256)],
)
def test_import_chunk_equals_import_rows(optim, dim, width):
    signs, inner = _signs(), _rows(width)
    whole, chunked = _store(optim, dim=dim), _store(optim, dim=dim)
    assert whole.row_width == width
    whole.import_rows(signs, inner)
    for lo in range(0, N_ROWS, 37):
        chunked.import_chunk(signs[lo:lo + 37], inner[lo:lo + 37])
    assert int(chunked._imported.item()) == N_ROWS
    assert chunked.finish_import() == 0
    ws, wi = _sorted(*whole.export_rows())
    cs, ci = _sorted(*chunked.export_rows())
    assert len(ws) == N_ROWS
    assert np.array_equal(cs, ws) and np.array_equal(ci, wi)
    es, ei = _sorted(signs, inner)
    assert np.array_equal(cs, es) and np.array_equal(ci, ei)


@pytest.mark.parametrize(
    "optim,src_width",
    [("sgd", 16),            # wider rows truncated (16 -> 8)
     ("adagrad", 8),         # state columns filled with the accumulator init
     ("adagrad_shared", 16), # 16 -> 9, narrow path
     ("adagrad", 9)],        # 9 -> 16, narrow path with fill
)
def test_import_chunk_adapts_row_width(optim, src_width):
    signs, inner = _signs(), _rows(src_width)
    store = _store(optim)
    state_init = float(store.optimizer.state_init(store.dim))
    if optim == "adagrad":
        assert state_init == pytest.approx(0.01)
    for lo in range(0, N_ROWS, 37):
        store.import_chunk(signs[lo:lo + 37], inner[lo:lo + 37])
    assert int(store._imported.item()) == N_ROWS
    assert store.finish_import() == 0
    want = _adapt_row_width(inner, store.row_width, state_init)
    gs, gi = _sorted(*store.export_rows())
    es, ei = _sorted(signs, np.ascontiguousarray(want))
    assert np.array_equal(gs, es) and np.array_equal(gi, ei)


def test_import_chunk_counts_dropped_rows():
    """A table whose every slot was touched at the chunk's own tick has no
    empty slot and no victim: each row of the chunk overflows, is dropped
    and counted, and nothing is written anywhere."""
    store = _store("sgd", capacity=64)
    keys = _craft(store, np.arange(store.n_slots))
    arena = store.arena.clone()
    store.ticks.fill_(store.tick)  # the tick import_chunk takes next
    signs, inner = _signs()[:100], _rows(8)[:100]
    store.import_chunk(signs, inner)
    assert int(store._imported.item()) == 0
    assert store.finish_import() == 100
    assert store.finish_import() == 0
    assert np.array_equal(store.keys.cpu().numpy().view(np.uint64), keys)
    assert torch.equal(store.arena, arena)
    # the next chunk has a new tick: every row evicts a victim and lands
    store.import_chunk(signs[:20], inner[:20])
    assert int(store._imported.item()) == 20
    assert store.finish_import() == 0


def test_import_chunk_with_spill_tier():
    from persia_amd.core.store import CpuEmbeddingStore
    from persia_amd.embedding import EmbeddingConfig

    signs, inner = _signs(), _rows(8)
    # condition of the input: the sequential oracle keeps every row
    cpu = CpuEmbeddingStore(8, 1024, _optim("sgd"), EmbeddingConfig(),
                            spill_capacity=4096)
    for lo in range(0, N_ROWS, 100):
        cpu.import_chunk(signs[lo:lo + 100], inner[lo:lo + 100])
    assert np.array_equal(np.sort(cpu.export_rows()[0]), np.sort(signs))

    store = _store("sgd", capacity=1024, spill_capacity=4096)
    assert store.n_slots == 1024
    for lo in range(0, N_ROWS, 100):
        store.import_chunk(signs[lo:lo + 100], inner[lo:lo + 100])
    assert store.finish_import() == 0
    store.flush_spill()
    assert len(store.spill) > 0
    gs, gi = _sorted(*store.export_rows())
    es, ei = _sorted(signs, inner)
    assert np.array_equal(gs, es) and np.array_equal(gi, ei)
    # and the streamed export walks HBM rows, then the spill rows
    _assert_same_export(store, 64)


# ------------------------------------------------------------ bounded memory


def test_export_chunks_memory_is_bounded_by_the_chunk():
    store = _store("adagrad", dim=128, capacity=1 << 16)
    assert store.n_slots == 1 << 16 and store.row_width == 256
    g = torch.Generator(device="cpu").manual_seed(11)
    occ = torch.randperm(store.n_slots, generator=g)[: store.n_slots // 2]
    keys = torch.zeros(store.n_slots, dtype=torch.int64)
    keys[occ] = torch.randint(1, 2 ** 62, (len(occ),), generator=g)
    store.keys.copy_(keys)
    store.arena.normal_()
    chunk = 1024
    torch.cuda.synchronize()

    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    n = 0
    for signs, _ in store.export_chunks(chunk):
        n += len(signs)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    assert n == store.n_slots // 2
    print(f"export_chunks peak rise: {rise} bytes")
    assert rise <= 2 * chunk * (4 * 256 + 8) + (1 << 20)

    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    signs, _ = store.export_rows()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    assert len(signs) == store.n_slots // 2
    print(f"export_rows peak rise: {rise} bytes")
    assert rise >= 32 << 20  # what the streaming path avoids


# ------------------------------------------------------------------- engine


def _engine():
    from persia_amd.core.engine import EmbeddingEngine
    from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
    from persia_amd.embedding import EmbeddingConfig

    return EmbeddingEngine(
        schema=EmbeddingSchema(
            slots={
                "a": SlotConfig(name="a", dim=16),
                "c": SlotConfig(name="c", dim=8),
            }
        ),
        hyper=EmbeddingConfig(),
        optimizer=_optim("adagrad"),
        gconf=GlobalConfig(capacity=1 << 12),
        device=_dev(),
        dist_ctx=DistContext(1, 0),
    )


def _batch():
    from persia_amd.embedding.data import IDTypeFeature, Label, PersiaBatch

    rng = np.random.default_rng(0)
    B = 32
    feats = [
        IDTypeFeature(n, [rng.integers(0, 300, size=4, dtype=np.uint64) for _ in range(B)])
        for n in ("a", "c")
    ]
    return PersiaBatch(feats, labels=[Label(np.ones((B, 1), np.float32))],
                       requires_grad=True)


def test_engine_stream_dump_and_load(tmp_path, monkeypatch):
    monkeypatch.setenv("PA_CKPT_CHUNK_ROWS", "37")
    eng = _engine()
    tb = eng.process_batch(_batch())
    eng.apply_gradients(
        tb,
        {
            "a": torch.full((32, 16), 0.5, dtype=torch.float16, device=_dev()),
            "c": torch.full((32, 8), -0.25, dtype=torch.float16, device=_dev()),
        },
    )
    monkeypatch.setenv("PA_CKPT_STREAM", "1")
    eng.dump(str(tmp_path / "stream"))
    monkeypatch.setenv("PA_CKPT_STREAM", "0")
    eng.dump(str(tmp_path / "legacy"))
    files = sorted(f for f in os.listdir(tmp_path / "legacy" / "s0") if f.endswith(".emb"))
    assert len(files) == 2
    for fn in files:
        a, b = tmp_path / "stream" / "s0" / fn, tmp_path / "legacy" / "s0" / fn
        assert os.path.getsize(a) > 32 + 37 * 8  # several chunks were streamed
        assert filecmp.cmp(str(a), str(b), shallow=False)

    monkeypatch.setenv("PA_CKPT_STREAM", "1")
    eng2 = _engine()
    eng2.load(str(tmp_path / "stream"))
    assert eng2.model_manager_status == "Idle"
    assert eng2.num_resident_rows() == eng.num_resident_rows() > 37
    tb1 = eng.process_batch(_batch(), train=False)
    tb2 = eng2.process_batch(_batch(), train=False)
    for p1, p2 in zip(tb1.payloads, tb2.payloads):
        assert torch.equal(p1.sum_tensor, p2.sum_tensor)
