"""Update hints: the lookup hands the fused sparse update each unique key's
slot and (for a key with one position) its gradient row, so the update can
skip the window probe and the ustarts/perm/seg_id walk.  Hints only shorten
the kernel's dependent loads: every result here is compared bit for bit with
the same call made without hints.

All tests are @pytest.mark.gpu."""
import numpy as np
import pytest
import torch

import test_gpu_kernels as K

pytestmark = pytest.mark.gpu

# dim -> kernel variant: 16 packed, 128 four keys per wave, 256 two keys per
# wave, 512 one key per wave
_DIMS = [16, 128, 256, 512]
_N_PAD = K._N_PAD


def _twins(dim, optname):
    case = K._fused_case(dim)
    wb = K._fused_bound(dim)
    a = K._hip_store(K._mk_opt(optname), dim=dim, weight_bound=wb)
    b = K._hip_store(K._mk_opt(optname), dim=dim, weight_bound=wb)
    for st in (a, b):
        st.lookup(case["looked_up"].to(K._dev()), train=True)
    assert torch.equal(a.arena, b.arena) and torch.equal(a.keys, b.keys)
    return case, a, b


def _true_hints(store, case):
    """What the lookup would emit for the case: slots from store_probe, the
    source row of every single-position key; the padding tail (never read)
    carries a hostile value."""
    from persia_amd.ops import native

    slot = native().store_probe(
        store.keys, store.ticks, case["uniq_pad"], int(store.tick),
        case["u_count"],
    ).clone()
    ustarts = case["ustarts_d"].cpu()
    perm, seg_id = case["perm"].cpu(), case["seg_id"].cpu()
    src = torch.full((_N_PAD,), 2**40, dtype=torch.int64)
    for u in range(K._N_UNIQ):
        lo, hi = int(ustarts[u]), int(ustarts[u + 1])
        s = int(seg_id[perm[lo]])
        src[u] = s if hi - lo == 1 and s >= 0 else -1
    slot[K._N_UNIQ:] = 2**40
    assert int(slot[K._U_MISSING]) == -1 and int(src[K._U_MULTI]) == -1
    return slot, src.to(K._dev())


def _step(store, case, slot_hint=None, src_hint=None):
    from persia_amd.ops import native

    powers = store._adam_step_powers()
    b1p, b2p = powers if powers else (0.0, 0.0)
    args = (
        store.keys, store.ticks, store.arena, case["uniq_pad"], case["grads"],
        case["perm"], case["ustarts_pad"], case["seg_id"], case["seg_scale"],
        store.dim, store._opt_code, store._opt_params(), float(b1p),
        float(b2p), float(store.hyper.weight_bound), store._skipped,
        case["u_count"],
    )
    if slot_hint is None:
        native().scatter_update(*args)
    else:
        native().scatter_update(*args, slot_hint, src_hint)


def _assert_same(hinted, plain):
    assert torch.equal(hinted.keys, plain.keys)
    assert torch.equal(hinted._skipped, plain._skipped)
    assert torch.equal(hinted.arena, plain.arena)
    assert plain._skipped.tolist() == [1, 1]  # one miss, one NaN row


@pytest.mark.parametrize("optname", K._FUSED_OPTS)
@pytest.mark.parametrize("dim", _DIMS)
def test_hinted_update_equals_unhinted(dim, optname):
    case, hinted, plain = _twins(dim, optname)
    slot, src = _true_hints(hinted, case)
    before = plain.arena.clone()
    _step(hinted, case, slot, src)
    _step(plain, case)
    _assert_same(hinted, plain)
    assert not torch.equal(plain.arena, before)  # the update did something


_HOSTILE = ["swapped", "empty_slot", "n_slots", "2**40", "-7",
            "never_inserted", "src_oob"]


@pytest.mark.parametrize("kind", _HOSTILE)
@pytest.mark.parametrize("dim", [16, 128])
def test_stale_and_hostile_hints(dim, kind):
    """A hint is a guess: out of range means no hint, a slot that does not
    hold the key falls back to the probe, and no row is ever stored through
    a hint that was not verified."""
    case, hinted, plain = _twins(dim, "adagrad")
    slot, src = _true_hints(hinted, case)
    n_slots = hinted.keys.numel()
    nan_row = None
    if kind == "swapped":  # two keys of one wave point at each other's row
        slot[[4, 5]] = slot[[5, 4]]
    elif kind == "empty_slot":
        empty = int((hinted.keys == 0).nonzero()[0])
        slot[4] = empty
    elif kind == "n_slots":
        slot[4] = n_slots
    elif kind == "2**40":
        slot[4] = 2**40
    elif kind == "-7":
        slot[4] = -7
    elif kind == "never_inserted":
        # the missing key claims the slot of a resident key whose own
        # gradient is NaN, so nothing may write that row at all
        slot[K._U_MISSING] = slot[K._U_NAN]
        nan_row = hinted.arena[int(slot[K._U_NAN])].clone()
    elif kind == "src_oob":  # one past the last gradient row
        src[4] = case["grads"].size(0)
    _step(hinted, case, slot, src)
    _step(plain, case)
    _assert_same(hinted, plain)
    if nan_row is not None:
        assert torch.equal(hinted.arena[int(slot[K._U_NAN])], nan_row)


def _engine(dim):
    from persia_amd.core.comm import DistContext
    from persia_amd.core.engine import EmbeddingEngine
    from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
    from persia_amd.embedding import EmbeddingConfig
    from persia_amd.embedding.optim import Adagrad

    return EmbeddingEngine(
        schema=EmbeddingSchema(
            slots={f"f{i}": SlotConfig(name=f"f{i}", dim=dim) for i in range(3)}
        ),
        hyper=EmbeddingConfig(emb_initialization=(-0.5, 0.5)),
        optimizer=Adagrad(lr=0.1),
        gconf=GlobalConfig(capacity=1 << 12),
        device=K._dev(),
        dist_ctx=DistContext(1, 0),
    )


def _batch(seed):
    from persia_amd.embedding.data import IDTypeFeatureWithSingleID, Label, PersiaBatch

    rng = np.random.default_rng(seed)
    feats = [
        IDTypeFeatureWithSingleID(f"f{i}", rng.integers(0, 50, size=32, dtype=np.uint64))
        for i in range(3)
    ]
    return PersiaBatch(feats, labels=[Label(np.ones((32, 1), np.float32))],
                       requires_grad=True)


@pytest.mark.parametrize("dim", [16, 128])
def test_lookup_emits_hints(dim):
    eng = _engine(dim)
    tb = eng.process_batch(_batch(0))
    torch.cuda.synchronize()
    g = tb._groups[0]
    assert g.slot_hint is not None and g.src_hint is not None
    U = int(g.u_count.item())
    assert 0 < U < 3 * 32  # ids in [0, 50): duplicates exist
    keys = eng.stores[dim].keys.cpu()
    uniq, slot, src = g.uniq_keys.cpu(), g.slot_hint.cpu(), g.src_hint.cpu()
    ustarts, perm, seg_id = g.ustarts.cpu(), g.perm.cpu(), g.seg_id.cpu()
    n_single = 0
    for u in range(U):
        s = int(slot[u])
        assert s == -1 or (0 <= s < keys.numel() and keys[s] == uniq[u]), u
        if int(ustarts[u + 1] - ustarts[u]) == 1:
            assert int(src[u]) == int(seg_id[perm[ustarts[u]]]), u
            n_single += 1
        else:
            assert int(src[u]) == -1, u
    assert 0 < n_single < U  # both kinds of key occurred
    assert int((slot[:U] >= 0).sum()) == U  # training lookup admits every key
    held = {t.data_ptr() for t in tb._device_tensors()}
    assert g.slot_hint.data_ptr() in held and g.src_hint.data_ptr() in held


@pytest.mark.parametrize("dim", [16, 128])
def test_engine_hints_on_off_same_bits(dim, monkeypatch):
    """The three-step loop of test_fused_scatter_update_matches_cpu with
    PA_UPDATE_HINTS=1 and =0 in fresh engines: the same arena."""
    arenas = []
    for knob in ("1", "0"):
        monkeypatch.setenv("PA_UPDATE_HINTS", knob)
        eng = _engine(dim)
        torch.manual_seed(7)
        for step in range(3):
            tb = eng.process_batch(_batch(step))
            grad = torch.randn(3 * 32, dim).to(torch.float16)
            tb.enable_training_views()
            tb._groups[0].sum_base.grad = grad.to(K._dev())
            eng.apply_gradients_base(tb)
        torch.cuda.synchronize()
        store = eng.stores[dim]
        assert store._skipped.tolist() == [0, 0]
        arenas.append((store.keys.clone(), store.arena.clone()))
    assert torch.equal(arenas[0][0], arenas[1][0])
    assert torch.equal(arenas[0][1], arenas[1][1])
