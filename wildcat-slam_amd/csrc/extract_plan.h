// extract_plan.h — the host-side decisions of a surfel extraction as plain C++17 (no HIP: g++ compiles it for the CPU tests,
// host/odom_c_api.cc): which pipeline a sweep starts on, which one repeats it when the device reports a flag, how large the
// tables and grids are, and the two halves of wc_ctx's extraction state.  extract.hip only launches what this header decides.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/wc_types.h"

struct wc_ctx;

constexpr int kBuckets = 4096;             // buckets of the composite sorts (points by voxel digit, surfels by time)
constexpr int kSlotBinMax = 512;           // surfels one time bin holds (k_slot_emit sorts a bin in LDS)
constexpr uint32_t kPtBinMax = 1024;       // runs per bucket the in-LDS path takes (4 wavefronts x 20 B x 1024 = 80 KB of LDS)
constexpr int kFxSub = 16;                 // default path: sub-counters (a single counter serialises at ~12 ns per atomic)
constexpr int kFxPts = 4, kFxThreads = 256, kFxTile = kFxPts * kFxThreads;  // default path: points per lane, lanes, points per tile

// Status bits a sweep's kernels raise (status word 1; mirrored into the pinned mailbox, word 8 + log2(bit))
constexpr uint32_t kFlagKeyRange = 1u;          // a point lies outside the key range around point 0 (+-512 root voxels; +-2^20 wide)
constexpr uint32_t kFlagSlotOverflow = 2u;      // more candidate clusters than slots (internal error)
constexpr uint32_t kFlagTimeRange = 4u;         // a surfel's stamp lies outside the [t_lo, t_hi] hint
constexpr uint32_t kFlagBucketOverflow = 8u;    // run-binned point sort: a bucket has more runs than its bin
constexpr uint32_t kFlagSlotBinOverflow = 16u;  // more than bin_cap surfels inside one 1/4096 of the time span
constexpr uint32_t kFlagLdsOverflow = 32u;      // run-binned point sort: a bucket fits its bin but not k_pt_bucket's LDS
constexpr uint32_t kFlagFxFallback = 64u;       // default path: a gate too close to its threshold, a table at capacity, ...
constexpr uint32_t kFlagsFxRepeat = kFlagFxFallback | kFlagKeyRange | kFlagSlotBinOverflow | kFlagTimeRange;  // default path -> exact path

// Which pipeline runs a sweep.
struct ExPath {
  bool fx = false;         // default integer-moment path (extract_fast.inc); the other three describe the exact path
  bool wide = false;       // 64-bit voxel keys (21 bits per axis) instead of 32-bit ones (10 bits)
  bool run_sort = false;   // run-binned point sort (k_pt_runs + k_pt_bucket) rather than the radix sort; never with wide keys
  bool bin_order = false;  // surfels ordered through time bins (k_slot_emit) rather than a radix sort of the slot keys
};
inline uint32_t ex_path_bits(const ExPath &p) { return (p.fx ? 1u : 0u) | (p.wide ? 2u : 0u) | (p.run_sort ? 4u : 0u) | (p.bin_order ? 8u : 0u); }

// The sweep in flight: written by enqueue, read by the tail and by finish().
struct ExSweep {
  bool active = false;         // enqueue was called, finish not yet
  wc_points pts{};             // the caller's points ...
  double t_lo = 0, t_hi = 0;   // ... the (widened) time hint ...
  wc_surfel *d_out = nullptr;  // ... and outputs (surfels, ids or null, capacity of both), kept for a repeat on another path
  wc_surfel_id *d_ids = nullptr;
  uint64_t cap = 0;
  ExPath path;                 // the pipeline the last enqueue of this sweep ran on
  uint32_t runs = 0;           // pipelines enqueued for this sweep so far (1: no repeat)
  uint32_t ticket = 0;         // ticket of the early count finish() waits for in the pinned mailbox (0: none - it waits for the stream)
  // the tail of the pipeline (layer-2 pass, surfel order, count / ticket) is run again by finish() when the enqueue skipped the
  // layer-2 launch and roots were queued for it after all
  int (*tail)(wc_ctx *, bool) = nullptr;
  bool layer2_done = true;     // the tail ran the layer-2 pass
  alignas(16) unsigned char roots_args[768];  // the pipeline's kernel arguments (RootsArgs or FxArgs, sizes included), for the tail
  unsigned slot_end_bit = 0;   // radix sort of the slot keys: bits that matter
  bool fx_split = false;       // default path: the node stage runs as k_fx_walk + k_fx_test (extract_split.inc)
  // batched extraction (wc_extract_surfels_batch_*): a sub-context prepares its sweep - tables, control block, kernel arguments
  // in roots_args - and leaves the launches to the parent, which runs K sweeps' kernels as one launch chain
  bool batch_defer = false;    // set by the batch enqueue around the sub-context's enqueue
  bool deferred = false;       // this sweep was prepared and waits for the batch's launches
};

// What a context remembers from sweep to sweep.
struct ExMemory {
  int general_calls = 0;         // upcoming sweeps that start on the radix point sort right away (set to 15 by a bucket overflow)
  uint32_t lds_cap = 256;        // runs per bucket k_pt_bucket sorts in LDS (256 / 512 / 1024: grows with the data, never shrinks)
  bool unordered = false;        // the previous run-sorted sweep had (almost) no run structure: stream with k_roots_banks
  uint32_t last_splits = 256;    // roots the previous sweep queued for the layer-2 pass (sizes / gates that launch)
  uint32_t fx_backoff = 0, fx_skip_calls = 0;  // default path: sweeps that go straight to the exact path after fall-backs (exponential)
  bool fx_long_lists = false, fx_long_lists2 = false;  // the last default-path sweep walked long record lists (2: in its layer-2 pass): k_fx_merge runs before k_fx_nodes
  bool fx_spill_full = false;    // the spill pool of the default path overflowed once: sized for the worst case from then on
  int fx_parity = 0;             // which of the default path's two control blocks the next sweep uses
  bool fx_dirty = false;         // the default path's tables may hold garbage (an aborted or repeated sweep): memset before the next use
  bool fx_ctrl_ready = false;    // the default path's two control blocks are initialised
  bool precleared = false;       // the exact path's control block has been cleared (on the stream) by the previous finish()
  bool bucket_attr_set = false;  // hipFuncSetAttribute(k_pt_bucket) done on this context's device
  uint32_t ticket_seq = 0;       // last ticket handed out (ex_mail_next_ticket)
  uint32_t fx_fallbacks = 0;     // sweeps the default path handed to the exact path so far
  uint32_t fx_last_flags = 0;    // status flags of the last default-path sweep
  uint32_t fx_last_why = 0;      // bit i: call site i of fx_fallback() fired in the last sweep that fell back
};

// new parameters or development options: the adaptive choice between default and exact path starts afresh
inline void ex_reset_backoff(ExMemory &m) { m.fx_backoff = m.fx_skip_calls = 0; }

// ---- the path of a sweep ---------------------------------------------------------------------------------------------------------
// enqueue's choice.  fx_ok: the default path takes this sweep (parameters, size, hint).  After a bucket overflow the next 15
// sweeps start on the radix point sort; after fall-backs the default path is skipped for fx_skip_calls sweeps.
inline ExPath ex_first_path(ExMemory &m, bool fx_ok, bool no_bucket_sort) {
  const bool general = m.general_calls > 0 || no_bucket_sort;
  if (m.general_calls > 0) --m.general_calls;
  if (fx_ok && m.fx_skip_calls > 0) --m.fx_skip_calls, fx_ok = false;
  return ExPath{fx_ok, false, !fx_ok && !general, true};
}

// finish's ladder: `flags` are the status bits of the run that just completed on `p` (`why_words`: the 24 mailbox words of the
// default path's reason codes, read only when it falls back).  true: p is the path to repeat the sweep on; false: the sweep stands as it is.  The
// checks keep their order - LDS, bucket, key range, slot bins - and every repeat is judged by its own fresh flags.
inline bool ex_next_path(ExPath &p, uint32_t flags, const uint32_t *why_words, ExMemory &m) {
  if (p.fx) {
    m.fx_last_flags = flags;
    if (!(flags & kFlagsFxRepeat)) {
      m.fx_backoff = 0;
      return false;
    }
    // a decision too close to its threshold, a table at capacity, a node spanning > 16 time bins, ...: repeat on the exact path
    ++m.fx_fallbacks;
    m.fx_last_why = 0;
    for (int i = 0; i < 24; ++i)
      if (why_words[i]) m.fx_last_why |= 1u << i;
    if (m.fx_last_why & (1u << 4)) m.fx_spill_full = true;  // the spill pool overflowed: full size from now on
    // exponential back-off: a sweep the default path cannot finish is usually followed by more of its kind; a gate that merely
    // fell inside the noise band is not
    m.fx_backoff = std::min(32u, std::max(1u, m.fx_backoff * 2u));
    m.fx_skip_calls = m.fx_backoff - 1u;
    m.fx_dirty = true;        // tables (a root at capacity, roots waiting for a layer-2 pass that never ran) ...
    m.fx_ctrl_ready = false;  // ... and control blocks are set up anew by the next default-path sweep
    // QUIRK, kept as it always behaved: ex_first_path chose the point sort from general_calls BEFORE its decrement and from
    // no_bucket_sort; this fall-back chooses it from general_calls AFTER the decrement and ignores the option.
    p = ExPath{false, false, !(m.general_calls > 0), true};
    return true;
  }
  if (p.run_sort) {  // (only the run-binned sort raises these two)
    bool bucket = flags & kFlagBucketOverflow;
    if ((flags & kFlagLdsOverflow) && !bucket && !(flags & kFlagKeyRange) && m.lds_cap < kPtBinMax) {
      m.lds_cap *= 2;  // a bucket had more runs than k_pt_bucket's LDS capacity (but fits its bin): one capacity up, sticky
      return true;
    }
    if (flags & kFlagLdsOverflow) bucket = true;  // still too large at the maximum
    if (bucket && !(flags & kFlagKeyRange)) {     // a bin of the run-binned point sort overflowed: radix sort, also for the next 15 sweeps
      p.run_sort = false;
      m.general_calls = 15;
      return true;
    }
  }
  if ((flags & kFlagKeyRange) && !p.wide) {  // more than +-512 root voxels around the first point: 21-bit-per-axis keys
    p.wide = true, p.run_sort = false;
    return true;
  }
  if ((flags & kFlagSlotBinOverflow) && p.bin_order) {  // very many surfels inside one 1/4096 of the time span: radix sort of the slot keys
    p.bin_order = false;
    return true;
  }
  return false;
}

// run statistics of the run-binned sort: fewer than four points per run on average = no run structure (a spinning multi-beam
// sensor in firing order): the next sweep streams with k_roots_banks right away
inline void ex_learn_unordered(ExMemory &m, const ExPath &p, uint32_t run_count, uint64_t n) {
  if (p.run_sort && run_count > 0) m.unordered = (uint64_t)run_count * 4 > n;
}

// ---- the early count: what k_slot_emit publishes as it starts and finish() waits for --------------------------------------------
// Surfel count, layer-2 queue length and the bin-overflow flag are final when k_slot_emit starts (functions of what the node stage
// left behind), so its last workgroup stores them to the pinned mailbox before it copies a surfel: two 64-bit words, each with the
// sweep's ticket in its upper half.  A word is one aligned store, so it is either the old word or the new one, and since each
// carries the ticket itself no order between the two is needed.  (constexpr: the kernel packs with the same functions.)
constexpr int kExMailTicket = 120;                 // 32-bit word of the pinned mailbox (ctx->h_status) where the two words start ...
constexpr int kExMailCount = kExMailTicket / 2;      // ... word A, as a 64-bit index: ticket << 32 | count
constexpr int kExMailQueue = kExMailTicket / 2 + 1;  // ... word B: ticket << 32 | overflow << 31 | queued
static_assert(kExMailTicket % 2 == 0, "the two words are 8-byte aligned");
constexpr uint64_t ex_mail_pack_count(uint32_t ticket, uint32_t count) { return ((uint64_t)ticket << 32) | count; }
// (a queue of 2^31 or more nodes cannot exist - the node blocks would not fit the card - and is reported as 2^31 - 1)
constexpr uint64_t ex_mail_pack_queue(uint32_t ticket, bool overflow, uint32_t queued) {
  return ((uint64_t)ticket << 32) | (overflow ? 0x80000000ull : 0ull) | (queued < 0x7FFFFFFFu ? queued : 0x7FFFFFFFu);
}
// both words are this sweep's (ticket 0 means "none" and never arrives; a stale ticket in either word is not arrival)
constexpr bool ex_mail_arrived(uint64_t a, uint64_t b, uint32_t ticket) {
  return ticket != 0u && (uint32_t)(a >> 32) == ticket && (uint32_t)(b >> 32) == ticket;
}
constexpr uint32_t ex_mail_count(uint64_t a) { return (uint32_t)a; }
constexpr uint32_t ex_mail_queued(uint64_t b) { return (uint32_t)b & 0x7FFFFFFFu; }
constexpr bool ex_mail_overflow(uint64_t b) { return ((uint32_t)b >> 31) != 0u; }
// the ticket after `seq`: the sequence skips 0 when it wraps
constexpr uint32_t ex_mail_next_ticket(uint32_t seq) { return seq + 1u != 0u ? seq + 1u : 1u; }

// ---- sizes -----------------------------------------------------------------------------------------------------------------------
// slots: the most surfels n points can give (`floor`: the default path hands slots out in kFxSub sub-ranges, never fewer than 256 each)
inline uint64_t ex_total_slots(uint64_t n, int max_layer, int cluster_min, uint64_t floor) {
  return std::max<uint64_t>((n * (uint64_t)(max_layer + 1)) / (uint64_t)cluster_min + 1, floor);
}
// capacity of a time bin: twice the count every bucket would get if EVERY slot held a surfel, 64 at least
inline uint32_t ex_slot_bin_cap(uint64_t total_slots) {
  uint32_t bin_cap = 64;
  while (bin_cap < (uint32_t)kSlotBinMax && (uint64_t)bin_cap * kBuckets < 2 * total_slots) bin_cap *= 2;
  return bin_cap;
}
inline unsigned ex_fx_tiles(uint64_t n) { return (unsigned)((n + kFxTile - 1) / kFxTile); }  // workgroups of k_fx_acc
// workgroups of k_fx_nodes<1> - and the blocks of the cluster-job buffer, which the layer-2 pass shares
inline unsigned ex_fx_node_grid(uint64_t n) { return std::min<unsigned>(256 * 16, std::max<unsigned>(64, (unsigned)(n / 256))); }
// ... of a sweep inside a batch: its node kernels loop over their sweep's parents, eight per wavefront (n / 256 blocks per sweep -
// what a single sweep's static hand-out wants - is 39 k workgroups for ten sweeps, 34 k of which find nothing to do)
inline unsigned ex_fx_batch_node_grid(uint64_t n) { return std::max(64u, ex_fx_node_grid(n) / 8u); }
// workgroups of the layer-2 node kernels: sized by the previous sweep's queue, within the sweep's node grid
inline unsigned ex_fx_layer2_grid(unsigned ngrid, uint32_t last_splits) { return std::min(std::min(256u * 8u, ngrid), std::max(64u, last_splits)); }
