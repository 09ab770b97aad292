"""Streaming checkpoint pipeline on the CPU backend: EmbFileWriter /
EmbFileReader against write_emb_file / read_emb_file, and the engine's
chunked dump/load against the whole-table path (PA_CKPT_STREAM=0), which
must produce byte-identical files."""
import filecmp
import os

import numpy as np
import pytest
import torch
import yaml

from persia_amd.core.checkpoint import (
    DONE_MARKER,
    EmbFileReader,
    EmbFileWriter,
    read_emb_file,
    write_emb_file,
)
from persia_amd.core.comm import DistContext
from persia_amd.core.engine import EmbeddingEngine
from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.data import IDTypeFeature, Label, PersiaBatch
from persia_amd.embedding.optim import Adagrad

ROW_WIDTH = 12


def _records(n):
    rng = np.random.default_rng(1234)
    signs = rng.integers(1, 2 ** 63, size=n, dtype=np.uint64)
    inner = rng.standard_normal((n, ROW_WIDTH)).astype(np.float32)
    return signs, inner


@pytest.mark.parametrize("n", [0, 1500])
@pytest.mark.parametrize("chunk", [1, 7, "n", "n+5"])
def test_writer_matches_write_emb_file(tmp_path, n, chunk):
    signs, inner = _records(n)
    chunk = {"n": max(1, n), "n+5": n + 5}.get(chunk, chunk)
    want = str(tmp_path / "want.emb")
    got = str(tmp_path / "got.emb")
    write_emb_file(want, signs, inner, dim=8)
    w = EmbFileWriter(got, n, 8, ROW_WIDTH)
    for lo in range(0, n, chunk):
        w.append(signs[lo:lo + chunk], inner[lo:lo + chunk])
    w.close()
    assert filecmp.cmp(want, got, shallow=False)


def test_writer_close_raises_on_short_count(tmp_path):
    signs, inner = _records(10)
    w = EmbFileWriter(str(tmp_path / "x.emb"), 10, 8, ROW_WIDTH)
    w.append(signs[:9], inner[:9])
    with pytest.raises(RuntimeError):
        w.close()


def test_writer_rejects_overflow(tmp_path):
    signs, inner = _records(10)
    w = EmbFileWriter(str(tmp_path / "x.emb"), 9, 8, ROW_WIDTH)
    with pytest.raises(ValueError):
        w.append(signs, inner)
    w.abort()


@pytest.mark.parametrize("n", [0, 1500])
@pytest.mark.parametrize("chunk", [1, 7, 1500, 1505])
def test_reader_chunks_concatenate_to_read_emb_file(tmp_path, n, chunk):
    signs, inner = _records(n)
    p = str(tmp_path / "x.emb")
    write_emb_file(p, signs, inner, dim=8)
    r = EmbFileReader(p)
    assert (r.n, r.dim, r.row_width) == (n, 8, ROW_WIDTH)
    parts = [(np.array(s), np.array(i)) for s, i in r.chunks(chunk)]
    assert all(0 < len(s) <= chunk and len(s) == len(i) for s, i in parts)
    got_s = np.concatenate([s for s, _ in parts]) if parts else np.zeros(0, np.uint64)
    got_i = (np.concatenate([i for _, i in parts]) if parts
             else np.zeros((0, ROW_WIDTH), np.float32))
    want_s, want_i, want_dim = read_emb_file(p)
    assert want_dim == r.dim
    assert np.array_equal(got_s, want_s)
    assert np.array_equal(got_i, want_i)


# ------------------------------------------------------------------ engine


def _engine():
    return EmbeddingEngine(
        schema=EmbeddingSchema(
            slots={
                "a": SlotConfig(name="a", dim=4),
                "c": SlotConfig(name="c", dim=8),
            }
        ),
        hyper=EmbeddingConfig(),
        optimizer=Adagrad(lr=0.1),
        gconf=GlobalConfig(capacity=1 << 12),
        device=torch.device("cpu"),
        dist_ctx=DistContext(1, 0),
    )


def _batch():
    rng = np.random.default_rng(0)
    feats = [
        IDTypeFeature("a", [rng.integers(0, 50, size=3, dtype=np.uint64) for _ in range(8)]),
        IDTypeFeature("c", [rng.integers(0, 50, size=2, dtype=np.uint64) for _ in range(8)]),
    ]
    return PersiaBatch(feats, labels=[Label(np.ones((8, 1), np.float32))], requires_grad=True)


def _trained_engine():
    eng = _engine()
    tb = eng.process_batch(_batch())
    eng.apply_gradients(
        tb,
        {
            "a": torch.full((8, 4), 0.5, dtype=torch.float16),
            "c": torch.full((8, 8), -0.25, dtype=torch.float16),
        },
    )
    return eng


def _emb_files(root):
    d = os.path.join(root, "s0")
    return sorted(fn for fn in os.listdir(d) if fn.endswith(".emb"))


def test_engine_stream_dump_is_byte_identical_to_legacy(tmp_path, monkeypatch):
    eng = _trained_engine()
    monkeypatch.setenv("PA_CKPT_CHUNK_ROWS", "5")
    monkeypatch.setenv("PA_CKPT_STREAM", "1")
    eng.dump(str(tmp_path / "stream"))
    monkeypatch.setenv("PA_CKPT_STREAM", "0")
    eng.dump(str(tmp_path / "legacy"))
    files = _emb_files(str(tmp_path / "legacy"))
    assert len(files) == 2 and files == _emb_files(str(tmp_path / "stream"))
    for fn in files:
        a = str(tmp_path / "stream" / "s0" / fn)
        b = str(tmp_path / "legacy" / "s0" / fn)
        assert EmbFileReader(a).n > 5  # more than one chunk was streamed
        assert filecmp.cmp(a, b, shallow=False)
    assert os.path.exists(str(tmp_path / "stream" / DONE_MARKER))
    assert os.path.exists(str(tmp_path / "stream" / "s0" / DONE_MARKER))


def test_engine_stream_load_roundtrip(tmp_path, monkeypatch):
    eng = _trained_engine()
    monkeypatch.setenv("PA_CKPT_CHUNK_ROWS", "5")
    monkeypatch.setenv("PA_CKPT_STREAM", "1")
    dst = str(tmp_path / "ckpt")
    eng.dump(dst)
    eng2 = _engine()
    eng2.load(dst)
    assert eng2.model_manager_status == "Idle"
    assert eng2.num_resident_rows() == eng.num_resident_rows()
    tb1 = eng.process_batch(_batch(), train=False)
    tb2 = eng2.process_batch(_batch(), train=False)
    for p1, p2 in zip(tb1.payloads, tb2.payloads):
        assert torch.equal(p1.sum_tensor, p2.sum_tensor)


@pytest.mark.parametrize("which", ["dump", "load"])
def test_engine_progress_is_monotonic_and_intermediate(tmp_path, monkeypatch, which):
    eng = _trained_engine()
    monkeypatch.setenv("PA_CKPT_CHUNK_ROWS", "5")
    monkeypatch.setenv("PA_CKPT_STREAM", "1")
    dst = str(tmp_path / "ckpt")
    if which == "load":
        eng.dump(dst)
        eng = _engine()
    seen = []
    orig = eng._set_status

    def spy(status, progress=0.0):
        seen.append((status, progress))
        orig(status, progress)

    monkeypatch.setattr(eng, "_set_status", spy)
    if which == "dump":
        eng.dump(dst)
        busy = "Dumping"
    else:
        eng.load(dst)
        busy = "Loading"
    assert seen[0] == (busy, 0.0) and seen[-1] == ("Idle", 100.0)
    assert all(s == busy for s, _ in seen[:-1])
    pct = [p for _, p in seen]
    assert all(a <= b for a, b in zip(pct, pct[1:]))
    assert any(0.0 < p < 100.0 for p in pct)


def test_dump_fails_when_streamed_count_differs(tmp_path, monkeypatch):
    """A store that yields fewer rows than its pre-count must fail the dump,
    not leave a short file behind a success status."""
    eng = _trained_engine()
    monkeypatch.setenv("PA_CKPT_STREAM", "1")
    store = eng.stores[8]
    orig = store.export_chunks

    def short(chunk_rows):
        it = orig(chunk_rows)
        signs, inner = next(it)
        yield signs[:-1], inner[:-1]

    monkeypatch.setattr(store, "export_chunks", short)
    with pytest.raises(RuntimeError):
        eng.dump(str(tmp_path / "ckpt"))
    assert eng.model_manager_status == "Failed"


def test_reshard_load_keeps_every_row(tmp_path, monkeypatch):
    """Two hand-built shard dirs (num_shards=2) into a world-1 engine."""
    monkeypatch.setenv("PA_CKPT_CHUNK_ROWS", "3")
    monkeypatch.setenv("PA_CKPT_STREAM", "1")
    rng = np.random.default_rng(7)
    signs = rng.integers(1, 2 ** 63, size=40, dtype=np.uint64)
    inner = rng.standard_normal((40, 16)).astype(np.float32)  # dim 8 + adagrad
    root = tmp_path / "ckpt"
    for r, sl in enumerate([slice(0, 23), slice(23, 40)]):
        d = root / f"s{r}"
        os.makedirs(d)
        write_emb_file(str(d / f"replica_{r}_shard_0.emb"), signs[sl], inner[sl], dim=8)
    with open(root / DONE_MARKER, "w", encoding="utf-8") as f:
        yaml.safe_dump({"num_shards": 2, "num_internal_shards": 1}, f)
    eng = _engine()
    eng.load(str(root))
    got_s, got_i = eng.stores[8].export_rows()
    order = np.argsort(got_s)
    want = np.argsort(signs)
    assert np.array_equal(got_s[order], signs[want])
    assert np.array_equal(got_i[order], inner[want])
    assert len(eng.stores[4]) == 0
