"""The sparse update kernels against the f64 optimizer models and per-element
bounds of tests/test_update_cases_cpu.py, from arbitrary (non-fresh) state.

Every run compares whole rows -- weights and optimizer state -- of every key
with the model run from the rows the kernel itself read, asserts both skip
counters exactly, and asserts that keys, ticks and every arena row the call
had no business writing (other keys' rows, the rows of missing and NaN keys)
are the same bits before and after.

Entry points: store_update (update_kernel); scatter_update without hints, with
a padded device-side count and with exact shapes; scatter_update with the
hints store_lookup_sums emits (also bit-equal to the unhinted twin);
HipEmbeddingStore.update_local for f16 gradients; update_local's fallback
(grad_scatter + store_update) for f32 and bf16 gradients and for dim 513.
Chains of four steps through the store API check each step from the rows the
previous step left, the beta powers, and that a stale power would be seen.

Worst err/bound measured on an MI355X (gfx950) per kernel family over all of
the tests below, and the plain unfused f32 loop of the CPU file beside it (on
that file's dims).  The figures near 1 are single roundings (a decayed
moment whose gradient is 0), where half an ulp is the bound itself:

    family                                   kernel   f32 loop
    update_kernel (store_update)             0.999    -
    grad_scatter + update_kernel (fallback)  1.000    0.994 (CPU store)
    scatter_update_kernel, packed dims       0.992    0.970
    scatter_update_multi_kernel<4>           0.994    0.987
    scatter_update_multi_kernel<2>           0.999    0.987
    scatter_update_kernel, one key per wave  1.000    0.996

(1.000 is a rounded 0.9996; no figure reaches 1.)  Hinted runs give the
figures of their unhinted twins, being the same bits.

All tests are @pytest.mark.gpu."""
import numpy as np
import pytest
import torch

import test_update_cases_cpu as UC

pytestmark = pytest.mark.gpu

_worst = {}   # family -> worst err/bound seen in this session (printed last)


def _dev():
    return torch.device("cuda", 0)


def _family(dim):
    if dim in UC.PACKED_DIMS:
        return "scatter_update_kernel (packed)"
    kpw = UC.keys_per_wave(dim)
    return {4: "scatter_update_multi_kernel<4>",
            2: "scatter_update_multi_kernel<2>",
            1: "scatter_update_kernel (one key)"}[kpw]


def _note(family, ratio):
    _worst[family] = max(_worst.get(family, 0.0), ratio)


def _store(case, capacity=4096, skip=()):
    """A table holding the case's resident rows (but `skip`) and the filler
    rows no update names, with the case's beta powers."""
    from persia_amd.core.store import HipEmbeddingStore
    from persia_amd.embedding import EmbeddingConfig

    store = HipEmbeddingStore(
        case.dim, capacity, case.opt,
        EmbeddingConfig(emb_initialization=(-0.5, 0.5), weight_bound=case.wb),
        _dev())
    keep = case.resident.copy()
    keep[list(skip)] = False
    if len(case.filler_signs):
        store.import_rows(case.filler_signs, case.filler_rows)
    store.import_rows(case.signs[keep], case.rows[keep])
    if case.powers:
        store.beta1_power, store.beta2_power = case.powers
    return store


_dev_cache = {}


def _on_device(case):
    """The call's tensors, uploaded once per case and shared read-only."""
    d = _dev_cache.get(id(case))
    if d is None:
        dev = _dev()
        d = dict(
            case=case,  # keeps id(case) alive
            uniq=torch.from_numpy(case.keys).to(dev),
            ustarts=torch.from_numpy(case.ustarts).to(dev),
            perm=torch.from_numpy(case.perm).to(dev),
            seg_id=torch.from_numpy(case.seg_id).to(dev),
            scale=(torch.from_numpy(case.seg_scale).to(dev)
                   if case.seg_scale is not None
                   else torch.empty(0, dtype=torch.float32, device=dev)),
            grads=case.grads.to(dev),
            u_count=torch.tensor([case.n], dtype=torch.int64, device=dev),
        )
        _dev_cache[id(case)] = d
    return d


def _slots(store, case):
    from persia_amd.ops import native

    d = _on_device(case)
    return native().store_probe(store.keys, store.ticks, d["uniq"][:case.n],
                                int(store.tick), store.no_count)


class _Before:
    def __init__(self, store, case):
        self.slots = _slots(store, case)
        self.keys = store.keys.clone()
        self.ticks = store.ticks.clone()
        self.arena = store.arena.clone()
        self.skipped = store._skipped.clone()
        self.resident = (self.slots >= 0).cpu().numpy()
        self.rows = self.arena[self.slots.clamp(min=0)].cpu().numpy()


def _check(store, case, before, family, powers=None, expect=None):
    """The call just made on `store` against the model run from `before`."""
    exp = expect or UC.model_step(case, before.rows, before.resident, powers)
    torch.cuda.synchronize()
    counters = (store._skipped - before.skipped).tolist()
    got = store.arena[before.slots.clamp(min=0)].cpu().numpy()
    ratio = UC.worst_ratio(got, exp.rows, rows=before.resident)
    print(f"{family} dim {case.dim} {case.optname} {case.gdtype}: "
          f"err/bound {ratio:.4f}, skips {counters}")
    assert counters == [exp.misses, exp.nans]
    assert ratio <= 1.0
    _note(family, ratio)
    # nothing else moved: keys, ticks, and every arena row but the stepped ones
    assert torch.equal(store.keys, before.keys)
    assert torch.equal(store.ticks, before.ticks)
    others = torch.ones(store.arena.size(0), dtype=torch.bool, device=_dev())
    others[before.slots[torch.from_numpy(exp.touched).to(_dev())]] = False
    assert torch.equal(store.arena[others], before.arena[others])
    quiet = before.resident & ~exp.touched  # NaN rows
    assert np.array_equal(got[quiet], before.rows[quiet])
    return exp


_model_cache = {}


def _one_step_model(case, before):
    """One-step tests all start from the imported rows: one model run per
    case."""
    assert np.array_equal(before.resident, case.resident)
    assert np.array_equal(before.rows[case.resident], case.rows[case.resident])
    if id(case) not in _model_cache:
        _model_cache[id(case)] = (case, UC.model_step(case, case.rows, case.resident))
    return _model_cache[id(case)][1]


def _scatter_update(store, case, padded=True, hints=None):
    from persia_amd.ops import native

    d = _on_device(case)
    n = case.n_pad if padded else case.n
    args = (store.keys, store.ticks, store.arena, d["uniq"][:n], d["grads"],
            d["perm"], d["ustarts"][:n + 1], d["seg_id"], d["scale"],
            *store._update_args(),
            d["u_count"] if padded else store.no_count)
    if hints is None:
        native().scatter_update(*args)
    else:
        native().scatter_update(*args, *hints)


def _emitted_hints(store, case):
    """(slot_hint, src_hint) of the case as a lookup emits them: from
    store_lookup_sums (no insert), slots cross-checked with store_probe."""
    from persia_amd.ops import native

    d = _on_device(case)
    sums = torch.empty(case.grads.shape[0], case.dim, dtype=torch.float16,
                       device=_dev())
    lo, hi = store.hyper.emb_initialization
    slot, src = native().store_lookup_sums(
        store.keys, store.ticks, store.arena, d["uniq"], d["perm"],
        d["ustarts"], sums, case.dim, 0, store.next_tick(), float(lo),
        float(hi), 1.0, float(store.optimizer.state_init(case.dim)),
        store.opt_space, d["u_count"], d["seg_id"])
    n = case.n
    assert torch.equal(slot[:n], _slots(store, case))
    lens = case.ustarts[1:n + 1] - case.ustarts[:n]
    first = case.seg_id[case.perm[case.ustarts[:n]]]
    want = np.where((lens == 1) & (first >= 0), first, -1)
    assert np.array_equal(src[:n].cpu().numpy(), want)
    assert (want >= 0).sum() > n // 2 and (want < 0).sum() >= 5
    return slot, src


_GRID = [(d, o) for d in UC.ALL_DIMS for o in UC.OPTS]


@pytest.mark.parametrize("padded", [True, False], ids=["u_count", "exact"])
@pytest.mark.parametrize("dim,optname", _GRID)
def test_scatter_update(dim, optname, padded):
    case = UC.cached_case(dim, optname)
    store = _store(case)
    before = _Before(store, case)
    _scatter_update(store, case, padded)
    _check(store, case, before, _family(dim),
           expect=_one_step_model(case, before))


@pytest.mark.parametrize("dim,optname", _GRID)
def test_scatter_update_hinted(dim, optname):
    """With the hints a lookup emits: within the bound, and the same bits as
    the twin store's unhinted call."""
    case = UC.cached_case(dim, optname)
    store, twin = _store(case), _store(case)
    hints = _emitted_hints(store, case)
    before = _Before(store, case)
    _scatter_update(store, case, True, hints)
    _scatter_update(twin, case, True)
    _check(store, case, before, _family(dim) + " hinted",
           expect=_one_step_model(case, before))
    # the claims of one import race, so the twins place keys differently:
    # compare key by key
    res = torch.from_numpy(case.resident).to(_dev())
    rows = [s.arena[_slots(s, case)[res]] for s in (store, twin)]
    assert torch.equal(rows[0].view(torch.int32), rows[1].view(torch.int32))
    assert torch.equal(twin._skipped, store._skipped)


_VARIANT_DIMS = (16, 128, 256, 512)  # one dim per kernel variant


@pytest.mark.parametrize("hinted", [False, True], ids=["plain", "hinted"])
@pytest.mark.parametrize("optname", UC.OPTS)
@pytest.mark.parametrize("dim", (2, 24) + _VARIANT_DIMS)
def test_update_local_f16(dim, optname, hinted):
    case = UC.cached_case(dim, optname)
    store = _store(case)
    d = _on_device(case)
    hints = _emitted_hints(store, case) if hinted else (None, None)
    before = _Before(store, case)
    store.update_local(d["grads"], d["perm"], d["ustarts"], d["seg_id"],
                       d["scale"], d["uniq"], d["u_count"], *hints)
    _check(store, case, before, _family(dim) + (" hinted" if hinted else ""),
           expect=_one_step_model(case, before))


@pytest.mark.parametrize("optname", UC.OPTS)
@pytest.mark.parametrize("dim", [1, 3, 8, 64, 129, 320, 513])
def test_store_update(dim, optname):
    """update_kernel on one f32 gradient row per key."""
    case = UC.cached_case(dim, optname, "f32", "rows")
    store = _store(case)
    d = _on_device(case)
    before = _Before(store, case)
    store.update_gradients(d["uniq"][:case.n], d["grads"])
    exp = _check(store, case, before, "update_kernel",
                 expect=_one_step_model(case, before))
    assert (exp.misses, exp.nans) == (1, 1)


@pytest.mark.parametrize("gdtype", ["f32", "bf16"])
@pytest.mark.parametrize("optname", UC.OPTS)
@pytest.mark.parametrize("dim", [8, 24, 320])
def test_update_local_fallback(dim, optname, gdtype):
    """f32 and bf16 gradients leave the fused kernel: a host read of the
    padded count, grad_scatter into an f32 buffer, then store_update."""
    case = UC.cached_case(dim, optname, gdtype, dyadic_betas=True)
    store = _store(case)
    d = _on_device(case)
    before = _Before(store, case)
    store.update_local(d["grads"], d["perm"], d["ustarts"], d["seg_id"],
                       d["scale"], d["uniq"], d["u_count"])
    _check(store, case, before, "grad_scatter + update_kernel",
           expect=_one_step_model(case, before))


def test_update_local_fallback_dim_513():
    """One past scatter_update's limit: f16 gradients, same fallback."""
    case = UC.cached_case(513, "adam")
    store = _store(case)
    d = _on_device(case)
    before = _Before(store, case)
    store.update_local(d["grads"], d["perm"], d["ustarts"], d["seg_id"],
                       d["scale"], d["uniq"], d["u_count"])
    _check(store, case, before, "grad_scatter + update_kernel",
           expect=_one_step_model(case, before))


# ------------------------------------------------------------------- chains

_N_FRESH = 30  # the last keys are not imported: the first lookup creates them
_CHAIN_STEPS = 4


@pytest.mark.parametrize("optname", UC.OPTS)
@pytest.mark.parametrize("dim", _VARIANT_DIMS)
def test_chain_of_steps(dim, optname):
    """Four update_local calls (odd steps plain, even steps hinted) on one
    store, new gradients each step.  Every step is checked from the rows the
    previous step left, so the per-step bound stays tight while the state is
    whatever the kernels produced; the 30 rows the lookup created start from
    the optimizer's initial state (Adagrad: accumulator 0)."""
    steps = [UC.make_case(dim, optname, seed=t, init_acc=0.0)
             for t in range(1, _CHAIN_STEPS + 1)]
    first = steps[0]
    fresh = range(first.n - _N_FRESH, first.n)
    store = _store(first, skip=fresh)
    if optname == "adam":  # a new store: the powers of step 1
        store.beta1_power, store.beta2_power = first.opt.betas
    d0 = _on_device(first)
    created = store.lookup(d0["uniq"][first.n - _N_FRESH:first.n], train=True)
    assert created.shape == (_N_FRESH, dim)
    if optname != "sgd":
        torch.cuda.synchronize()
        rows = _Before(store, first).rows[first.n - _N_FRESH:]
        assert (rows[:, dim:] == 0).all()
    b1, b2 = first.opt.betas if optname == "adam" else (None, None)
    p1, p2 = b1, b2
    for t, case in enumerate(steps, start=1):
        assert np.array_equal(case.keys, first.keys)
        d = _on_device(case)
        hints = _emitted_hints(store, case) if t % 2 == 0 else (None, None)
        before = _Before(store, case)
        powers = None
        if optname == "adam":
            powers = (store.beta1_power, store.beta2_power)
            assert powers == (p1, p2)
        store.update_local(d["grads"], d["perm"], d["ustarts"], d["seg_id"],
                           d["scale"], d["uniq"], d["u_count"], *hints)
        _check(store, case, before, _family(dim) + " chain", powers=powers)
        if optname == "adam":
            # the chain can see a stale power: beta^(t-1) does not match
            stale = UC.model_step(case, before.rows, before.resident,
                                  powers=(p1 / b1, p2 / b2))
            got = store.arena[before.slots.clamp(min=0)].cpu().numpy()
            assert UC.worst_ratio(got, stale.rows, rows=before.resident) > 1.0
            p1, p2 = p1 * b1, p2 * b2
        _dev_cache.pop(id(case), None)
    if optname == "adam":
        assert (store.beta1_power, store.beta2_power) == (p1, p2)
        assert p1 == b1 * b1 * b1 * b1 * b1
    assert store._skipped.tolist() == [_CHAIN_STEPS, 2 * _CHAIN_STEPS]


# -------------------------------------------------------------- grid stride


def _stride_store(spec):
    case = UC.stride_case(spec["dim"], spec["n"])
    store = _store(case, capacity=spec["capacity"])
    before = _Before(store, case)
    lost = int((~before.resident).sum())
    assert 1 <= lost < 0.01 * case.n  # the missing key, and insert overflow
    return case, store, before


def test_store_update_grid_stride():
    """More keys than 16384 blocks of four waves: update_kernel's grid-stride
    loop takes a second trip."""
    case, store, before = _stride_store(UC.STRIDE_UPDATE)
    assert case.n > 16384 * 4
    d = _on_device(case)
    store.update_gradients(d["uniq"][:case.n], d["grads"])
    _check(store, case, before, "update_kernel")
    _dev_cache.pop(id(case), None)


def test_scatter_update_grid_stride():
    """More than 16384 * 4 * 4 keys at dim 3: the four-key kernel's loop."""
    case, store, before = _stride_store(UC.STRIDE_QUAD)
    assert case.n > 16384 * 4 * 4
    _scatter_update(store, case, True)
    _check(store, case, before, "scatter_update_multi_kernel<4>")
    _dev_cache.pop(id(case), None)


def test_zz_report_worst_ratios():
    """Not a check of its own: prints what this session measured."""
    for family in sorted(_worst):
        print(f"worst err/bound  {family:48s} {_worst[family]:.4f}")
