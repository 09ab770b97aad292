// Native lookup/update drivers: the per-batch hot path of the embedding
// engine as single C++ calls (the reference's forward/backward engines are
// native Rust; here the orchestration of sign-prep -> dedup -> probe ->
// init/gather -> fused segment-sum (and scatter -> fused optimizer on the
// way back) is C++ driving the HIP kernels + rocPRIM sort via ATen, so the
// pipeline thread does one extension call instead of ~25 Python dispatches).
//
// The distributed path keeps its all_to_all hops in Python (they go through
// torch.distributed process groups); it reuses the pieces exposed here.
#include <torch/extension.h>

// kernels.hip entry points
void store_lookup(torch::Tensor table_keys, torch::Tensor ticks,
                  torch::Tensor arena, torch::Tensor query, torch::Tensor out,
                  int64_t dim, int64_t train, int64_t tick, double lo,
                  double hi, double admit_prob, double state_init,
                  int64_t opt_space, torch::Tensor evict_keys,
                  torch::Tensor evict_count, torch::Tensor evict_rows,
                  torch::Tensor u_count);
std::vector<torch::Tensor> store_lookup_sums(
    torch::Tensor table_keys, torch::Tensor ticks, torch::Tensor arena,
    torch::Tensor query, torch::Tensor perm, torch::Tensor ustarts,
    torch::Tensor sums, int64_t dim, int64_t train, int64_t tick, double lo,
    double hi, double admit_prob, double state_init, int64_t opt_space,
    torch::Tensor u_count, torch::Tensor seg_id);
std::vector<torch::Tensor> bag_plan(torch::Tensor plan, int64_t S, int64_t B,
                                    int64_t nnz, torch::Tensor sqrt_flags);
std::vector<torch::Tensor> store_lookup_bags(
    torch::Tensor table_keys, torch::Tensor ticks, torch::Tensor arena,
    torch::Tensor query, torch::Tensor inverse, torch::Tensor perm,
    torch::Tensor ustarts, torch::Tensor cat_offsets, torch::Tensor seg_scale,
    torch::Tensor sums, int64_t dim, int64_t train, int64_t tick, double lo,
    double hi, double admit_prob, double state_init, int64_t opt_space,
    torch::Tensor u_count, torch::Tensor seg_id);
std::vector<torch::Tensor> raw_plan(torch::Tensor plan, int64_t S, int64_t B,
                                    int64_t nnz, torch::Tensor sqrt_flags,
                                    torch::Tensor raw_meta,
                                    std::vector<int64_t> sfs);
std::vector<torch::Tensor> store_lookup_raw(
    torch::Tensor table_keys, torch::Tensor ticks, torch::Tensor arena,
    torch::Tensor query, torch::Tensor inverse, torch::Tensor perm,
    torch::Tensor ustarts, torch::Tensor cat_offsets, torch::Tensor seg_scale,
    torch::Tensor plan, torch::Tensor raw_meta, std::vector<int64_t> sfs,
    int64_t S, int64_t B, torch::Tensor base, torch::Tensor mask, int64_t dim,
    int64_t train, int64_t tick, double lo, double hi, double admit_prob,
    double state_init, int64_t opt_space, torch::Tensor u_count,
    torch::Tensor seg_id);
void store_update(torch::Tensor table_keys, torch::Tensor ticks,
                  torch::Tensor arena, torch::Tensor query,
                  torch::Tensor grads, int64_t dim, int64_t opt,
                  std::vector<double> params, double b1_power,
                  double b2_power, double weight_bound, torch::Tensor skipped);
torch::Tensor segment_sum(torch::Tensor rows, torch::Tensor inverse,
                          torch::Tensor seg_offsets, torch::Tensor seg_scale);
void grad_scatter(torch::Tensor grads, torch::Tensor perm,
                  torch::Tensor ustarts, torch::Tensor seg_id,
                  torch::Tensor seg_scale, torch::Tensor out,
                  int64_t accumulate);
torch::Tensor sign_prep(torch::Tensor values, torch::Tensor slot_starts,
                        torch::Tensor prefixes, int64_t spacing);
torch::Tensor sign_prep_bags(torch::Tensor upload, int64_t nnz_in,
                             int64_t nnz_out, int64_t S, int64_t B,
                             torch::Tensor prefixes, torch::Tensor rounds,
                             torch::Tensor sizes, int64_t spacing);
void scatter_update(torch::Tensor table_keys, torch::Tensor ticks,
                    torch::Tensor arena, torch::Tensor uniq,
                    torch::Tensor grads, torch::Tensor perm,
                    torch::Tensor ustarts, torch::Tensor seg_id,
                    torch::Tensor seg_scale, int64_t dim, int64_t opt,
                    std::vector<double> params, double b1_power,
                    double b2_power, double weight_bound,
                    torch::Tensor skipped, torch::Tensor u_count,
                    torch::Tensor slot_hint, torch::Tensor src_hint);
void dedup_finalize(torch::Tensor svals_flipped, torch::Tensor perm,
                    torch::Tensor neq, torch::Tensor rank, int64_t flip,
                    torch::Tensor inverse, torch::Tensor uniq,
                    torch::Tensor ustarts, torch::Tensor u_count);
std::vector<torch::Tensor> sort_pairs_u64(torch::Tensor keys);
torch::Tensor neq_flags(torch::Tensor sorted);

static constexpr int64_t kFlip = std::numeric_limits<int64_t>::min();

// sort-based dedup (torch.sort on GPU = rocPRIM radix/merge sort).
// -> (uniq ascending u64-order, inverse, perm, ustarts)
std::vector<torch::Tensor> dedup_keys(torch::Tensor keys) {
  auto dev = keys.device();
  const int64_t nnz = keys.numel();
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(dev);
  if (nnz == 0) {
    auto z = torch::zeros({0}, opts);
    return {z, z, z, torch::zeros({1}, opts)};
  }
  auto flipped = keys.bitwise_xor(kFlip);
  auto sorted = flipped.sort();
  auto svals = std::get<0>(sorted);
  auto perm = std::get<1>(sorted);
  auto neq = torch::ones({nnz}, opts.dtype(torch::kBool));
  neq.slice(0, 1, nnz) =
      svals.slice(0, 1, nnz).ne(svals.slice(0, 0, nnz - 1));
  auto inv_sorted = neq.cumsum(0) - 1;
  auto inverse = torch::empty({nnz}, opts);
  inverse.index_put_({perm}, inv_sorted);
  auto uniq = svals.masked_select(neq).bitwise_xor(kFlip);
  auto starts = neq.nonzero().view(-1);
  auto ustarts = torch::cat({starts, torch::full({1}, nnz, opts)});
  return {uniq, inverse, perm, ustarts};
}

// Fixed-shape dedup: every tensor is nnz-padded and the true unique count
// lives ONLY on the device (u_count) — no host synchronization anywhere, so
// the pipeline thread issues the whole batch and returns (a
// masked_select/nonzero dedup forces two stream syncs per batch,
// serializing the producer behind the GPU).  The uniq tail is ZERO-filled
// (the empty-key sentinel, which sign prep never produces), so consumers
// that do scan past u_count probe an impossible key.
// -> {uniq zeros-padded [nnz], inverse [nnz], perm [nnz],
//     ustarts padded [nnz+1], u_count device i64[1]}
std::vector<torch::Tensor> dedup_padded(torch::Tensor keys) {
  const int64_t nnz = keys.numel();
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(keys.device());
  // u64 radix sort needs no sign-flip: unsigned order IS key/owner order
  auto sp = sort_pairs_u64(keys);
  auto& svals = sp[0];
  auto& perm = sp[1];
  auto neq = neq_flags(svals);
  auto rank = neq.cumsum(0);
  rank.sub_(1);
  auto inverse = torch::empty({nnz}, opts);
  auto uniq = torch::zeros({nnz}, opts);
  // dedup_finalize launches nothing for an empty input, so the empty result
  // (no unique keys, ustarts = [0]) is written here
  auto ustarts = nnz ? torch::empty({nnz + 1}, opts) : torch::zeros({1}, opts);
  auto u_count = nnz ? torch::empty({1}, opts) : torch::zeros({1}, opts);
  dedup_finalize(svals, perm, neq, rank, /*flip=*/0, inverse, uniq, ustarts,
                 u_count);
  return {uniq, inverse, perm, ustarts, u_count};
}

// Single-GPU fused lookup: raw values -> per-sample summed embeddings.
// Returns {sums f16 [n_segs, dim], uniq_keys, inverse, perm, ustarts,
// u_count, slot_hint, src_hint}; the last two are the update hints of
// store_lookup_sums, computed from the group's seg_id (position -> gradient
// row) and handed back to update_local.
std::vector<torch::Tensor> lookup_local(
    torch::Tensor values, torch::Tensor slot_starts, torch::Tensor prefixes,
    int64_t spacing, torch::Tensor cat_offsets, torch::Tensor seg_scale,
    torch::Tensor seg_id, torch::Tensor table_keys, torch::Tensor ticks,
    torch::Tensor arena, int64_t dim, int64_t train, int64_t tick, double lo,
    double hi, double admit_prob, double state_init, int64_t opt_space) {
  auto keys = sign_prep(values, slot_starts, prefixes, spacing);
  auto d = dedup_padded(keys);
  auto& uniq = d[0];
  auto& inverse = d[1];
  auto& perm = d[2];
  auto& ustarts = d[3];
  auto& u_count = d[4];
  const int64_t nnz = keys.numel();
  auto dev = values.device();
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(dev);
  // the all-single-ID fast path has exactly one id per segment
  // (cat_offsets is the identity partition), so the sum rows are a pure
  // per-position scatter of the unique rows: fuse init+gather+f16-cast into
  // one kernel and skip the [nnz, dim] f32 intermediate entirely
  auto sums = torch::empty(
      {nnz, dim}, torch::TensorOptions().dtype(torch::kFloat16).device(dev));
  auto hints = store_lookup_sums(table_keys, ticks, arena, uniq, perm, ustarts,
                                 sums, dim, train, tick, lo, hi, admit_prob,
                                 state_init, opt_space, u_count, seg_id);
  return {sums, uniq, inverse, perm, ustarts, u_count, hints[0], hints[1]};
}

// The bag lookup behind sign prep: padded dedup -> segment plan ->
// probe/claim -> init launch (training) -> sums straight from the arena.
// `plan` is slot_starts[S+1] ‖ offsets[S, B+1] over the keys' positions.
static std::vector<torch::Tensor> bags_from_keys(
    torch::Tensor keys, torch::Tensor plan, int64_t S, int64_t B,
    torch::Tensor sqrt_flags, int64_t hints, torch::Tensor table_keys,
    torch::Tensor ticks, torch::Tensor arena, int64_t dim, int64_t train,
    int64_t tick, double lo, double hi, double admit_prob, double state_init,
    int64_t opt_space) {
  auto d = dedup_padded(keys);
  auto& uniq = d[0];
  auto& inverse = d[1];
  auto& perm = d[2];
  auto& ustarts = d[3];
  auto& u_count = d[4];
  auto p = bag_plan(plan, S, B, keys.numel(), sqrt_flags);
  auto& cat_offsets = p[0];
  auto& seg_id = p[1];
  auto sums = torch::empty(
      {S * B, dim},
      torch::TensorOptions().dtype(torch::kFloat16).device(keys.device()));
  const bool want_hints = train && hints;
  auto h = store_lookup_bags(
      table_keys, ticks, arena, uniq, inverse, perm, ustarts, cat_offsets,
      p[3], sums, dim, train, tick, lo, hi, admit_prob, state_init, opt_space,
      u_count, want_hints ? seg_id : seg_id.narrow(0, 0, 0));
  return {sums,       uniq, inverse,     perm,   ustarts, u_count,
          h[0],       h[1], cat_offsets, seg_id, p[2],    p[3]};
}

// Single-GPU fused lookup of a bag group: sum slots with any number of ids per
// sample.  `upload` is the group's one H2D buffer,
//   values[nnz] ‖ slot_starts[S+1] ‖ offsets[S, B+1]
// (offsets per slot, relative to the slot's start, checked by the host
// builder).  sign prep -> padded dedup -> segment plan -> probe/claim -> init
// launch (training) -> sums straight from the arena.  No host sync, no
// [U, dim] row buffer.  sqrt_flags i32[S] marks the sqrt-scaling slots, empty
// when there is none; hints != 0 asks for the update hints (training only).
// Returns {sums f16 [S*B, dim], uniq, inverse, perm, ustarts, u_count,
// slot_hint, src_hint, cat_offsets, seg_id, seg_lens, seg_scale}; seg_scale
// is empty (all ones) without a sqrt slot, the hints are empty unless asked.
std::vector<torch::Tensor> lookup_local_bags(
    torch::Tensor upload, int64_t nnz, int64_t S, int64_t B,
    torch::Tensor prefixes, int64_t spacing, torch::Tensor sqrt_flags,
    int64_t hints, torch::Tensor table_keys, torch::Tensor ticks,
    torch::Tensor arena, int64_t dim, int64_t train, int64_t tick, double lo,
    double hi, double admit_prob, double state_init, int64_t opt_space) {
  TORCH_CHECK(S >= 1 && B >= 0 && nnz >= 0 &&
                  upload.scalar_type() == torch::kInt64 &&
                  upload.is_contiguous() &&
                  upload.numel() == nnz + S + 1 + S * (B + 1),
              "lookup_local_bags: upload must be i64[nnz + S+1 + S*(B+1)]");
  TORCH_CHECK(prefixes.numel() == S, "lookup_local_bags: prefixes must be [S]");
  // sign_prep, the dedup epilogue and probe_claim run one thread per position
  // on a grid capped at 16384 blocks of 256: beyond that they would leave
  // positions unwritten
  TORCH_CHECK(nnz <= (int64_t)16384 * 256,
              "lookup_local_bags: ", nnz, " ids in one dim-group, the "
              "thread-per-position kernels cover 4194304");
  auto values = upload.narrow(0, 0, nnz);
  auto slot_starts = upload.narrow(0, nnz, S + 1);
  auto plan = upload.narrow(0, nnz, S + 1 + S * (B + 1));
  auto keys = sign_prep(values, slot_starts, prefixes, spacing);
  return bags_from_keys(keys, plan, S, B, sqrt_flags, hints, table_keys, ticks,
                        arena, dim, train, tick, lo, hi, admit_prob, state_init,
                        opt_space);
}

// lookup_local_bags for a group with hashstack slots (a stacked sum slot is a
// bag: each id becomes R bucketed ids inside its sample's span).  `upload` is
//   values[nnz_in] ‖ slot_starts[S+1] ‖ offsets[S, B+1] ‖ in_starts[S+1]
// with slot_starts and offsets in the expanded space of nnz_out positions and
// the ids unexpanded (engine pack_stack_bag_buffer); rounds i32[S] / sizes
// i64[S] are the device constants of sign_prep_bags, rounds_host / sizes_host
// the same values for the checks made here, without a sync.  Behind sign
// prep the chain is lookup_local_bags' on nnz_out positions; the twelve
// results are sized by nnz_out.
std::vector<torch::Tensor> lookup_local_bags_stack(
    torch::Tensor upload, int64_t nnz_in, int64_t nnz_out, int64_t S,
    int64_t B, torch::Tensor prefixes, int64_t spacing,
    torch::Tensor sqrt_flags, torch::Tensor rounds, torch::Tensor sizes,
    std::vector<int64_t> rounds_host, std::vector<int64_t> sizes_host,
    int64_t hints, torch::Tensor table_keys, torch::Tensor ticks,
    torch::Tensor arena, int64_t dim, int64_t train, int64_t tick, double lo,
    double hi, double admit_prob, double state_init, int64_t opt_space) {
  TORCH_CHECK(S >= 1 && B >= 0 && nnz_in >= 0 && nnz_out >= 0 &&
                  upload.scalar_type() == torch::kInt64 &&
                  upload.is_contiguous() &&
                  upload.numel() == nnz_in + 2 * (S + 1) + S * (B + 1),
              "lookup_local_bags_stack: upload must be "
              "i64[nnz_in + S+1 + S*(B+1) + S+1]");
  TORCH_CHECK(prefixes.numel() == S,
              "lookup_local_bags_stack: prefixes must be [S]");
  TORCH_CHECK(rounds.numel() == S && sizes.numel() == S &&
                  (int64_t)rounds_host.size() == S &&
                  (int64_t)sizes_host.size() == S,
              "lookup_local_bags_stack: rounds and sizes must be [S] (", S,
              "), got ", rounds.numel(), ", ", sizes.numel(), ", ",
              rounds_host.size(), ", ", sizes_host.size());
  int64_t max_rounds = 1;
  for (int64_t s = 0; s < S; ++s) {
    TORCH_CHECK(rounds_host[s] >= 0, "lookup_local_bags_stack: slot ", s,
                " has ", rounds_host[s], " hashstack rounds");
    TORCH_CHECK(rounds_host[s] == 0 || sizes_host[s] >= 1,
                "lookup_local_bags_stack: slot ", s, " has embedding_size ",
                sizes_host[s]);
    max_rounds = std::max(max_rounds, rounds_host[s]);
  }
  // the per-slot split of nnz_in is on the device only: hold nnz_out to what
  // the totals allow
  TORCH_CHECK(nnz_out >= nnz_in && nnz_out <= nnz_in * max_rounds,
              "lookup_local_bags_stack: ", nnz_out, " positions from ", nnz_in,
              " ids of at most ", max_rounds, " rounds");
  // the thread-per-position limit of lookup_local_bags, on the expanded count
  TORCH_CHECK(nnz_out <= (int64_t)16384 * 256,
              "lookup_local_bags_stack: ", nnz_out, " positions in one "
              "dim-group, the thread-per-position kernels cover 4194304");
  auto plan = upload.narrow(0, nnz_in, S + 1 + S * (B + 1));
  auto keys = sign_prep_bags(upload, nnz_in, nnz_out, S, B, prefixes, rounds,
                             sizes, spacing);
  return bags_from_keys(keys, plan, S, B, sqrt_flags, hints, table_keys, ticks,
                        arena, dim, train, tick, lo, hi, admit_prob, state_init,
                        opt_space);
}

// Single-GPU fused lookup of a raw group: S sum slots (single-ID or bags),
// then R = sfs.size() raw (sequence) slots, whose output is the fixed-size
// tensor [B, sfs[r], dim] and a 0/1 mask per cell.  `upload` is the group's
// one H2D buffer in lookup_local_bags' layout over all S+R slots,
//   values[nnz] ‖ slot_starts[S+R+1] ‖ offsets[S+R, B+1]
// raw_meta is the device copy of row_base[R] ‖ sfs[R] (raw_plan).  sign prep
// -> padded dedup -> plan -> probe/claim -> init launch (training) -> sums,
// then the raw cells, both straight from the arena.  No host sync.  A
// position past sfs in its sample is looked up and inserted like any other; it
// feeds no cell and its seg_id is -1.
// Returns {base f16 [S*B + sum_r B*sfs[r], dim] (sums, then each raw slot's
// cell rows, sample-major), mask f16 [sum_r B*sfs[r]], uniq, inverse, perm,
// ustarts, u_count, slot_hint, src_hint, cat_offsets, seg_id, seg_lens,
// seg_scale, raw_num}: cat_offsets and seg_lens cover the sum region, seg_id
// all positions; seg_scale covers base's rows (1 over the raw rows) or is empty
// without a sqrt slot; raw_num i64[R*B] is min(len, sfs) per raw sample.
std::vector<torch::Tensor> lookup_local_raw(
    torch::Tensor upload, int64_t nnz, int64_t S, int64_t B,
    torch::Tensor prefixes, int64_t spacing, torch::Tensor sqrt_flags,
    torch::Tensor raw_meta, std::vector<int64_t> sfs, int64_t hints,
    torch::Tensor table_keys, torch::Tensor ticks, torch::Tensor arena,
    int64_t dim, int64_t train, int64_t tick, double lo, double hi,
    double admit_prob, double state_init, int64_t opt_space) {
  const int64_t R = (int64_t)sfs.size();
  const int64_t n_slots = S + R;
  TORCH_CHECK(S >= 0 && R >= 1 && B >= 0 && nnz >= 0 &&
                  upload.scalar_type() == torch::kInt64 &&
                  upload.is_contiguous() &&
                  upload.numel() == nnz + n_slots + 1 + n_slots * (B + 1),
              "lookup_local_raw: upload must be "
              "i64[nnz + S+R+1 + (S+R)*(B+1)]");
  TORCH_CHECK(prefixes.numel() == n_slots,
              "lookup_local_raw: prefixes must be [S+R]");
  // the thread-per-position limit of lookup_local_bags
  TORCH_CHECK(nnz <= (int64_t)16384 * 256,
              "lookup_local_raw: ", nnz, " ids in one dim-group, the "
              "thread-per-position kernels cover 4194304");
  auto values = upload.narrow(0, 0, nnz);
  auto slot_starts = upload.narrow(0, nnz, n_slots + 1);
  auto plan = upload.narrow(0, nnz, n_slots + 1 + n_slots * (B + 1));
  auto keys = sign_prep(values, slot_starts, prefixes, spacing);
  auto d = dedup_padded(keys);
  auto& uniq = d[0];
  auto& inverse = d[1];
  auto& perm = d[2];
  auto& ustarts = d[3];
  auto& u_count = d[4];
  auto p = raw_plan(plan, S, B, nnz, sqrt_flags, raw_meta, sfs);
  auto& cat_offsets = p[0];
  auto& seg_id = p[1];
  int64_t n_cells = 0;
  for (int64_t f : sfs) n_cells += B * f;
  auto f16 =
      torch::TensorOptions().dtype(torch::kFloat16).device(upload.device());
  auto base = torch::empty({S * B + n_cells, dim}, f16);
  auto mask = torch::empty({n_cells}, f16);
  const bool want_hints = train && hints;
  auto h = store_lookup_raw(
      table_keys, ticks, arena, uniq, inverse, perm, ustarts, cat_offsets,
      p[3], plan, raw_meta, sfs, S, B, base, mask, dim, train, tick, lo, hi,
      admit_prob, state_init, opt_space, u_count,
      want_hints ? seg_id : seg_id.narrow(0, 0, 0));
  return {base, mask, uniq,        inverse, perm, ustarts, u_count,
          h[0], h[1], cat_offsets, seg_id,  p[2], p[3],    p[4]};
}

// Single-GPU fused backward: per-segment grads -> per-sign scatter -> fused
// optimizer update on the shard.
void update_local(torch::Tensor grads, torch::Tensor perm,
                  torch::Tensor ustarts, torch::Tensor seg_id,
                  torch::Tensor seg_scale, torch::Tensor uniq_keys,
                  torch::Tensor table_keys, torch::Tensor ticks,
                  torch::Tensor arena, int64_t dim, int64_t opt,
                  std::vector<double> params, double b1_power, double b2_power,
                  double weight_bound, torch::Tensor skipped,
                  torch::Tensor u_count, torch::Tensor slot_hint,
                  torch::Tensor src_hint) {
  if (grads.scalar_type() == torch::kFloat16 && dim <= 512) {
    // single fused kernel: ordered scatter + optimizer, no [U,dim] buffer
    scatter_update(table_keys, ticks, arena, uniq_keys, grads, perm, ustarts,
                   seg_id, seg_scale, dim, opt, params, b1_power, b2_power,
                   weight_bound, skipped, u_count, slot_hint, src_hint);
    return;
  }
  // rare fallback (f32 grads or dim > 512): needs exact shapes — for a
  // padded (device-count) dedup, pay the one host sync and slice
  if (u_count.numel()) {
    const int64_t U = u_count.item<int64_t>();
    uniq_keys = uniq_keys.narrow(0, 0, U);
    ustarts = ustarts.narrow(0, 0, U + 1);
  }
  auto buf = torch::empty(
      {uniq_keys.numel(), dim},
      torch::TensorOptions().dtype(torch::kFloat32).device(grads.device()));
  grad_scatter(grads, perm, ustarts, seg_id, seg_scale, buf, /*accumulate=*/0);
  store_update(table_keys, ticks, arena, uniq_keys, buf, dim, opt, params,
               b1_power, b2_power, weight_bound, skipped);
}


// ---------------------------------------------------------------- host tier
// Host-DRAM spill tier (native): rows evicted from the HBM table park here
// and come back on their next lookup.  Exclusive bounded LRU with
// insert-order recency, matching persia_amd/core/store.py HostTier (the
// python oracle) exactly: re-insert refreshes recency, fetch removes, the
// oldest entry is dropped past capacity.  Replaces per-key python dict
// loops in the pipeline thread (reference: remote CPU parameter-server
// shards, embedding_parameter_server/lib.rs).
#include <list>
#include <memory>
#include <unordered_map>
#include <vector>

struct NativeHostTier {
  // Row payloads live in fixed-size slabs with a free-list (two heap
  // allocations PER INSERT — list node + row vector — dominated the
  // original implementation and fragmented the host heap at 1e8-row
  // scale); the key map is sharded 16 ways so rehash pauses are 1/16th
  // the size.  LRU stays one global list of (key, slot).
  static constexpr int64_t CHUNK_ROWS = 1 << 16;
  static constexpr int SHARDS = 16;
  int64_t capacity, row_width;
  std::vector<std::unique_ptr<float[]>> chunks;
  std::vector<int64_t> free_slots;
  int64_t next_fresh = 0;  // slots handed out so far (before any free)
  std::list<std::pair<uint64_t, int64_t>> lru;  // (key, slot); front = oldest
  std::unordered_map<uint64_t,
                     std::list<std::pair<uint64_t, int64_t>>::iterator>
      map[SHARDS];

  NativeHostTier(int64_t cap, int64_t rw) : capacity(cap), row_width(rw) {}

  float* rowp(int64_t slot) {
    return chunks[slot / CHUNK_ROWS].get() + (slot % CHUNK_ROWS) * row_width;
  }
  int64_t alloc_slot() {
    if (!free_slots.empty()) {
      const int64_t s = free_slots.back();
      free_slots.pop_back();
      return s;
    }
    if (next_fresh >= (int64_t)chunks.size() * CHUNK_ROWS)
      chunks.emplace_back(new float[CHUNK_ROWS * row_width]);
    return next_fresh++;
  }
  auto& shard(uint64_t key) { return map[key & (SHARDS - 1)]; }

  void erase_entry(std::list<std::pair<uint64_t, int64_t>>::iterator it) {
    free_slots.push_back(it->second);
    shard(it->first).erase(it->first);
    lru.erase(it);
  }

  void insert(torch::Tensor keys, torch::Tensor rows) {
    TORCH_CHECK(!keys.is_cuda() && !rows.is_cuda(), "HostTier: cpu tensors");
    TORCH_CHECK(rows.size(1) == row_width, "HostTier: row width mismatch");
    auto kc = keys.contiguous();
    auto rc = rows.contiguous();
    const int64_t* kp = kc.data_ptr<int64_t>();
    const float* rp = rc.data_ptr<float>();
    const int64_t k = kc.numel();
    for (int64_t i = 0; i < k; ++i) {
      const uint64_t key = (uint64_t)kp[i];
      auto& m = shard(key);
      auto it = m.find(key);
      int64_t slot;
      if (it != m.end()) {  // refresh: reuse the slot, move to back
        slot = it->second->second;
        lru.erase(it->second);
        lru.emplace_back(key, slot);
        it->second = std::prev(lru.end());
      } else {
        slot = alloc_slot();
        lru.emplace_back(key, slot);
        m[key] = std::prev(lru.end());
      }
      std::copy(rp + i * row_width, rp + (i + 1) * row_width, rowp(slot));
    }
    while ((int64_t)lru.size() > capacity) erase_entry(lru.begin());
  }

  std::tuple<torch::Tensor, torch::Tensor> fetch(torch::Tensor keys) {
    auto kc = keys.contiguous();
    const int64_t* kp = kc.data_ptr<int64_t>();
    const int64_t k = kc.numel();
    auto rows = torch::zeros({k, row_width}, torch::kFloat32);
    auto found = torch::zeros({k}, torch::kBool);
    float* rp = rows.data_ptr<float>();
    bool* fp = found.data_ptr<bool>();
    for (int64_t i = 0; i < k; ++i) {
      const uint64_t key = (uint64_t)kp[i];
      auto& m = shard(key);
      auto it = m.find(key);
      if (it == m.end()) continue;
      const float* src = rowp(it->second->second);
      std::copy(src, src + row_width, rp + i * row_width);
      fp[i] = true;
      erase_entry(it->second);
    }
    return {rows, found};
  }

  std::tuple<torch::Tensor, torch::Tensor> export_all() {
    const int64_t n = (int64_t)lru.size();
    auto keys = torch::empty({n}, torch::kInt64);
    auto rows = torch::empty({n, row_width}, torch::kFloat32);
    int64_t* kp = keys.data_ptr<int64_t>();
    float* rp = rows.data_ptr<float>();
    int64_t i = 0;
    for (auto& e : lru) {
      kp[i] = (int64_t)e.first;
      const float* src = rowp(e.second);
      std::copy(src, src + row_width, rp + i * row_width);
      ++i;
    }
    return {keys, rows};
  }

  int64_t size() const { return (int64_t)lru.size(); }
  bool contains(int64_t key) {
    return shard((uint64_t)key).count((uint64_t)key) != 0;
  }
  void clear() {
    lru.clear();
    for (auto& m : map) m.clear();
    chunks.clear();
    free_slots.clear();
    next_fresh = 0;
  }
};

void init_engine(pybind11::module_& m) {
  m.def("dedup_keys", &dedup_keys, "sort-based dedup of u64 keys");
  m.def("dedup_padded", &dedup_padded,
        "sync-free dedup: nnz-padded outputs + device unique count");
  pybind11::class_<NativeHostTier>(m, "HostTier")
      .def(pybind11::init<int64_t, int64_t>())
      .def("insert", &NativeHostTier::insert)
      .def("fetch", &NativeHostTier::fetch)
      .def("export_all", &NativeHostTier::export_all)
      .def("size", &NativeHostTier::size)
      .def("contains", &NativeHostTier::contains)
      .def("clear", &NativeHostTier::clear);
  m.def("lookup_local", &lookup_local,
        "fused single-GPU lookup (sign prep + dedup + probe + gather + sum)");
  m.def("lookup_local_bags", &lookup_local_bags,
        "fused single-GPU lookup of a multi-ID sum group (sign prep + dedup + "
        "segment plan + probe + init + sums from the arena)");
  m.def("lookup_local_bags_stack", &lookup_local_bags_stack,
        "lookup_local_bags for a group with hashstack slots (sign prep "
        "expands the unexpanded ids on the device)");
  m.def("lookup_local_raw", &lookup_local_raw,
        "fused single-GPU lookup of a group with raw (sequence) slots (sign "
        "prep + dedup + plan + probe + init + sums and raw cells from the "
        "arena)");
  m.def("update_local", &update_local,
        "fused single-GPU backward (scatter + optimizer update)");
}
