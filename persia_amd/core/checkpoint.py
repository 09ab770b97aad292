"""Embedding checkpoint dump/load.

Directory layout mirrors the reference model manager
(persia-model-manager/src/lib.rs:124-240):

    dst/
      s0/ replica_0_shard_0.emb ...
      s1/ ...
      embedding_dump_done          <- yaml marker {num_shards,
                                      num_internal_shards, datetime}

The reference's speedy-serialized ArrayLinkedList framing is replaced by a
documented little-endian record format (the speedy submodule is not
verifiable — SURVEY §5 Checkpoint note):

    file   := magic "PAEMB1\\0\\0" | u64 num_records | u64 embedding_dim
              | u64 row_width
              | u64 signs[num_records]                  (columnar: all signs)
              | f32 inner[num_records * row_width]      (then all rows)
    inner row = emb(dim) ‖ opt_state — reference emb_entry.rs:17-23 layout.
    All fields little-endian; the two arrays are contiguous blocks, NOT
    interleaved per record.

Dump and load stream the table through fixed-size chunks
(EmbFileWriter / EmbFileReader + the stores' export_chunks / import_chunk),
so the extra memory is O(chunk) whatever the table size; PA_CKPT_STREAM=0
selects the whole-table path, which writes the same bytes.

Re-sharding on load when the dumped shard count differs from the current
world size mirrors mod.rs:1150-1259: every rank scans all files and keeps the
signs it owns.
"""
import datetime
import os
import struct
from typing import TYPE_CHECKING, Iterator, Tuple

import numpy as np
import yaml

from persia_amd.core import hashing
from persia_amd.logger import get_default_logger

if TYPE_CHECKING:
    from persia_amd.core.engine import EmbeddingEngine

_logger = get_default_logger("persia_amd.checkpoint")

_MAGIC = b"PAEMB1\x00\x00"
DONE_MARKER = "embedding_dump_done"


def write_emb_file(path: str, signs: np.ndarray, inner: np.ndarray, dim: int) -> None:
    n, row_width = inner.shape
    assert len(signs) == n
    with open(path, "wb") as f:
        f.write(_MAGIC)
        f.write(struct.pack("<QQQ", n, dim, row_width))
        f.write(np.ascontiguousarray(signs, dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(inner, dtype=np.float32).tobytes())


def read_emb_file(path: str) -> Tuple[np.ndarray, np.ndarray, int]:
    with open(path, "rb") as f:
        magic = f.read(8)
        assert magic == _MAGIC, f"bad .emb magic in {path}"
        n, dim, row_width = struct.unpack("<QQQ", f.read(24))
        signs = np.frombuffer(f.read(8 * n), dtype=np.uint64).copy()
        inner = (
            np.frombuffer(f.read(4 * n * row_width), dtype=np.float32)
            .reshape(n, row_width)
            .copy()
        )
    return signs, inner, int(dim)


_HEADER_BYTES = len(_MAGIC) + 24


def stream_enabled() -> bool:
    """PA_CKPT_STREAM (default 1): 0 keeps the whole-table dump/load."""
    return os.environ.get("PA_CKPT_STREAM", "1") != "0"


def chunk_rows_for(row_width: int) -> int:
    """PA_CKPT_CHUNK_ROWS, default sized for ~256 MiB per staging buffer."""
    env = os.environ.get("PA_CKPT_CHUNK_ROWS")
    if env:
        return max(1, int(env))
    return max(1024, (256 << 20) // (4 * max(1, row_width)))


def _pwrite_all(fd: int, buf, offset: int) -> None:
    view = memoryview(buf).cast("B")
    while len(view):
        w = os.pwrite(fd, view, offset)
        view = view[w:]
        offset += w


class EmbFileWriter:
    """Incremental writer of one .emb file.  The record count is fixed up
    front, so the signs block and the rows block each have a known start and
    ``append`` writes a chunk at the two running offsets; nothing is buffered
    beyond the caller's chunk."""

    def __init__(self, path: str, n: int, dim: int, row_width: int):
        self.path = path
        self.n = int(n)
        self.dim = int(dim)
        self.row_width = int(row_width)
        self.written = 0
        self._fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        _pwrite_all(
            self._fd,
            _MAGIC + struct.pack("<QQQ", self.n, self.dim, self.row_width), 0,
        )
        self._signs_off = _HEADER_BYTES
        self._rows_off = _HEADER_BYTES + 8 * self.n

    def append(self, signs: np.ndarray, inner: np.ndarray) -> None:
        k = len(signs)
        if inner.shape != (k, self.row_width):
            raise ValueError(
                f"{self.path}: chunk shape {inner.shape} != ({k}, {self.row_width})"
            )
        if self.written + k > self.n:
            raise ValueError(
                f"{self.path}: {self.written + k} records appended, header says {self.n}"
            )
        if k == 0:
            return
        _pwrite_all(
            self._fd, np.ascontiguousarray(signs, dtype=np.uint64),
            self._signs_off + 8 * self.written,
        )
        _pwrite_all(
            self._fd, np.ascontiguousarray(inner, dtype=np.float32).reshape(-1),
            self._rows_off + 4 * self.row_width * self.written,
        )
        self.written += k

    def close(self) -> None:
        if self._fd is None:
            return
        os.close(self._fd)
        self._fd = None
        if self.written != self.n:
            raise RuntimeError(
                f"{self.path}: {self.written} records written, header says {self.n}"
            )

    def abort(self) -> None:
        """Close without the count check (an error is already propagating)."""
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None


class EmbFileReader:
    """Chunked reader of one .emb file: the two columnar blocks are memory
    mapped and ``chunks`` yields read-only views, so only the pages of the
    chunk in flight are resident."""

    def __init__(self, path: str):
        self.path = path
        with open(path, "rb") as f:
            magic = f.read(8)
            assert magic == _MAGIC, f"bad .emb magic in {path}"
            n, dim, row_width = struct.unpack("<QQQ", f.read(24))
        self.n, self.dim, self.row_width = int(n), int(dim), int(row_width)
        need = _HEADER_BYTES + 8 * self.n + 4 * self.n * self.row_width
        assert os.path.getsize(path) >= need, f"truncated .emb file {path}"

    def chunks(self, chunk_rows: int) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
        chunk_rows = max(1, int(chunk_rows))
        if self.n == 0:
            return
        signs = np.memmap(
            self.path, dtype="<u8", mode="r", offset=_HEADER_BYTES, shape=(self.n,)
        )
        if self.row_width:
            inner = np.memmap(
                self.path, dtype="<f4", mode="r",
                offset=_HEADER_BYTES + 8 * self.n, shape=(self.n, self.row_width),
            )
        else:
            inner = np.zeros((self.n, 0), dtype=np.float32)
        for lo in range(0, self.n, chunk_rows):
            hi = min(self.n, lo + chunk_rows)
            yield signs[lo:hi], inner[lo:hi]


def _write_markers(engine: "EmbeddingEngine", dst_dir: str, shard_dir: str,
                   n_dims: int) -> None:
    rank = engine.dist.rank
    # replica-level marker
    with open(os.path.join(shard_dir, DONE_MARKER), "w", encoding="utf-8") as f:
        yaml.safe_dump(
            {
                "num_shards": engine.dist.world_size,
                "num_internal_shards": n_dims,
                "datetime": datetime.datetime.now().isoformat(),
            },
            f,
        )
    engine.dist_grad.barrier()
    if rank == 0:
        with open(os.path.join(dst_dir, DONE_MARKER), "w", encoding="utf-8") as f:
            yaml.safe_dump(
                {
                    "num_shards": engine.dist.world_size,
                    "num_internal_shards": n_dims,
                    "datetime": datetime.datetime.now().isoformat(),
                },
                f,
            )
    engine.dist_grad.barrier()


def _store_record_count(store) -> int:
    """Records a dump of ``store`` holds: resident rows plus spilled rows."""
    flush = getattr(store, "flush_spill", None)
    if flush is not None:
        flush()
    n = len(store)
    if store.spill is not None:
        n += len(store.spill)
    return n


def dump_embedding(engine: "EmbeddingEngine", dst_dir: str) -> None:
    rank = engine.dist.rank
    shard_dir = os.path.join(dst_dir, f"s{rank}")
    os.makedirs(shard_dir, exist_ok=True)
    dims = sorted(engine.stores.keys())
    if not stream_enabled():
        for shard_idx, dim in enumerate(dims):
            signs, inner = engine.stores[dim].export_rows()
            path = os.path.join(shard_dir, f"replica_{rank}_shard_{shard_idx}.emb")
            write_emb_file(path, signs, inner, dim)
        _write_markers(engine, dst_dir, shard_dir, len(dims))
        return
    # The table must not be mutated during a dump: the header carries the
    # pre-count, and a streamed count that differs makes close() raise.
    counts = {dim: _store_record_count(engine.stores[dim]) for dim in dims}
    total = sum(counts.values())
    done = 0
    for shard_idx, dim in enumerate(dims):
        store = engine.stores[dim]
        path = os.path.join(shard_dir, f"replica_{rank}_shard_{shard_idx}.emb")
        writer = EmbFileWriter(path, counts[dim], dim, store.row_width)
        try:
            for signs, inner in store.export_chunks(chunk_rows_for(store.row_width)):
                writer.append(signs, inner)
                done += len(signs)
                engine._set_status("Dumping", 100.0 * min(done, total) / max(1, total))
        except BaseException:
            writer.abort()
            raise
        writer.close()
    _write_markers(engine, dst_dir, shard_dir, len(dims))


def load_embedding(engine: "EmbeddingEngine", src_dir: str) -> None:
    marker = os.path.join(src_dir, DONE_MARKER)
    assert os.path.exists(marker), f"no {DONE_MARKER} marker in {src_dir}"
    with open(marker, "r", encoding="utf-8") as f:
        info = yaml.safe_load(f)
    num_shards = int(info["num_shards"])
    rank, world = engine.dist.rank, engine.dist.world_size
    streaming = stream_enabled()

    def import_file(path: str, filter_owner: bool):
        signs, inner, dim = read_emb_file(path)
        if dim not in engine.stores:
            _logger.warning(f"checkpoint dim {dim} has no configured slots; skipping {path}")
            return
        if filter_owner and world > 1:
            owner = hashing.owner_of(hashing.splitmix64(signs), world)
            keep = owner == rank
            signs, inner = signs[keep], inner[keep]
        if len(signs):
            engine.stores[dim].import_rows(signs, inner)

    if num_shards == world:
        files = [(os.path.join(src_dir, f"s{rank}"), False)]
    else:
        # re-shard: scan every replica dir, keep owned signs
        files = [(os.path.join(src_dir, f"s{r}"), True) for r in range(num_shards)]
    paths = [
        (os.path.join(shard_dir, fn), filter_owner)
        for shard_dir, filter_owner in files
        for fn in sorted(os.listdir(shard_dir))
        if fn.endswith(".emb")
    ]
    if not streaming:
        for path, filter_owner in paths:
            import_file(path, filter_owner)
        engine.dist_grad.barrier()
        return

    readers = [(EmbFileReader(path), filter_owner) for path, filter_owner in paths]
    total = sum(r.n for r, _ in readers)
    done = 0
    touched = []
    for reader, filter_owner in readers:
        store = engine.stores.get(reader.dim)
        if store is None:
            _logger.warning(
                f"checkpoint dim {reader.dim} has no configured slots; skipping {reader.path}"
            )
            done += reader.n
            continue
        if store not in touched:
            touched.append(store)
        for signs, inner in reader.chunks(chunk_rows_for(store.row_width)):
            k = len(signs)
            if filter_owner and world > 1:
                # host-side owner filter, before the copy to the device
                owner = hashing.owner_of(hashing.splitmix64(np.asarray(signs)), world)
                keep = owner == rank
                signs, inner = signs[keep], inner[keep]
            if len(signs):
                store.import_chunk(signs, inner)
            done += k
            engine._set_status("Loading", 100.0 * done / max(1, total))
    for store in touched:
        finish = getattr(store, "finish_import", None)
        dropped = finish() if finish is not None else 0
        if dropped:
            _logger.warning(
                f"checkpoint load: {dropped} rows of dim {store.dim} found no free "
                f"slot and were dropped (table over capacity)"
            )
    engine.dist_grad.barrier()
