// extract_fast.inc — the DEFAULT extraction path: order-independent integer moments (included by extract.hip inside its
// anonymous namespace; it shares ExParams, the surfel slots, the time bins and k_slot_emit with the exact path).
//
// The exact path (k_pt_runs .. k_roots_emit above) forms every moment sum in the order the reference forms it
// (surfel_extraction.cc:36-47, :89-97) - a dependent fp64 addition per point and wavefront, which pins the stage to the
// latency floor.  north_star asks for bit-exact voxel indices / surfel counts and 1e-6 on the surfel geometry; SURVEY Q6
// already prescribes "flag near-threshold nodes".  This path therefore
//   * accumulates the moments of every (root voxel, layer-1 octant, time bin) CELL as 64-bit INTEGERS of the point
//     coordinates relative to the (1/1024 m rounded) voxel centre in units of 2^-32 m, and of t - t_lo in units of 2^-s s:
//     integer addition is associative, so any reduction shape - lanes, LDS atomics, HBM atomics, any input order, any number
//     of tiles - gives the same sums, which are exact to ~1e-14 (the reference's un-centred fp64 sums carry ~1e-12 of
//     cancellation noise, SURVEY Q6);
//   * finds the temporal clusters of a node (ClusterSurfels, cc:22-29: a new cluster where consecutive points of the node
//     are more than 0.05 s apart) from the first / last timestamp of its time bins (bin width < 0.05 s, so a gap can only
//     open between bins) - again order independent;
//   * takes every decision the reference takes (n > 20, n >= 20, lambda_0 < 0.01f, likeness > 0.1, cc:33,54,106-111,129,172)
//     on these sums, and raises kFlagFxFallback whenever a PCA gate is closer to its threshold than the reference's own
//     rounding noise or this path's own grids could move it: finish() then repeats the sweep on the exact path.  Counts and ids are therefore the
//     reference's; centre / covariance / normal / sigma agree with the exact values to the grids' rounding (covariance entries 2^-45 m^2,
//     bounds and measurements per field: DESIGN.md 4.3, tests/test_extract_precision_gpu.py); a surfel's timestamp is the correctly rounded mean
//     (the reference's running sum rounds at ~1e-5 s with epoch-sized stamps), so the OUTPUT ORDER - ascending timestamp,
//     ties by id - can differ from the exact path's where two surfels are closer in time than that noise.
// Kernels (C2: 3 launches):
//   k_fx_acc<1>    ONE pass over the points: 4 consecutive points per lane, per-lane integer partial sums while the cell
//                  stays the same, LDS hash of the tile's cells (ds atomics); every cell of the tile becomes ONE 128-byte
//                  record in HBM (plain stores) that is pushed onto the cell's list in its root's block with ONE atomic
//                  exchange; roots get a dense index through an insert-only hash table.  Its phases overlap: the per-point part
//                  (fx_point) runs per load round while the later rounds are in flight, its results go through LDS to the lane that
//                  owns four consecutive points; the direct records are linked (fx_link_claim, fx_link_head) as soon as the cell
//                  codes are known and stored (fx_store) when their sums exist.  Development option fx_acc_form selects the forms
//                  without either part (k_fx_acc_form<LEVEL, FORM>): every form writes the same bytes
//   k_fx_nodes<1>  8 lanes per root voxel (lane = layer-1 octant), 8 roots per wavefront: every lane walks the record lists
//                  of its node in time-bin order - node totals, temporal clusters -, then node tests and cluster PCAs
//                  (cc:82-126, :12-65), emission into slots + time bins, layer-2 queue, list heads cleaned behind it
//   k_fx_acc<2> / k_fx_nodes<2>   the same pair for the layer-2 children of the queued layer-1 nodes (cc:170-183)
//   k_slot_emit    (shared) time order + copy to the caller's buffer
// All tables are zero at rest: k_fx_nodes clears what k_fx_acc touched (list heads, block headers, hash entries) and
// k_slot_emit clears the control block of the next sweep (two blocks, used alternately), so a sweep pays neither a bulk memset
// nor a clean-up launch.

// (kFxPts consecutive points per lane, kFxThreads, kFxTile, kFxSub sub-counters: extract_plan.h)
constexpr int kFxLds = 256;        // cells of the per-tile LDS hash
constexpr int kFxLdsProbe = 12;
constexpr int kFxDirect = 16;     // records a wavefront may write straight to HBM per flush class (3 in-lane boundaries + run tails)
constexpr int kFxRecTile = kFxLds + (kFxThreads / 64) * 4 * kFxDirect;  // record slots per tile: hash cells | direct records per wavefront
constexpr int kFxSlots = 16;       // time slots per node: bin & 15
constexpr int kFxRecW = 16;        // u64 words per record (128 B): n | bin << 32, St, Sq[3], Sqq[6], tmin_inv, tmax_p1, next, 2 spare
constexpr int kFxHdrW = 16;        // u64 words of a block header
constexpr int kFxBlockW = kFxHdrW + 8 * kFxSlots / 2;  // + 128 list heads (u32): 80 words = 640 B per root / per queued node
// Counter banks (roots created, layer-2 nodes queued, surfel slots taken, spill records): 16 sub-counters each, every one on
// its own 128-byte line - atomics on different words of ONE line serialise like atomics on one word (~11 ns each).
constexpr uint32_t kFxStRoots = 0, kFxStNodes2 = 1, kFxStSlots = 2, kFxStSpillBank = 3;
constexpr int kFxCntStride = 32;  // u32 words between two sub-counters
constexpr int kFxCntWords = 4 * kFxSub * kFxCntStride;
constexpr unsigned long long kFxTMax = 0xFFFFFFFFFFFFull;  // ticks are < 2^41
// magic numbers of k_fx_acc's integer moments (see its pass A): 1.5 x 2^52 (integers in the low mantissa bits) and 1.5 x 2^72 (multiples
// of 2^20); the low words of their bit patterns are zero, so n x bits(M) only touches a sum's high word
constexpr double kFxMagic = 6755399441055744.0, kFxMagic2 = 7083549724304467820544.0;
constexpr unsigned long long kFxMagicBits = 0x4338000000000000ull;
constexpr uint32_t kFxMagicHi = 0x43380000u, kFxMagic2Hi = 0x44780000u;

struct FxArgs {
  wc_points pts;
  ExParams P;
  double t_lo;       // widened lower time bound (ticks and bins are relative to it)
  double tick, inv_tick;   // 2^s, 2^-s
  double inv_w;      // 1 / bin width
  double inv_span;   // 1 / (t_hi - t_lo): time keys of the surfel order are 32-bit fractions of the sweep
  double inv_vs;     // 1 / (double)voxel_size: estimate of the voxel index, confirmed by the true division near integers
  double qs, inv_q, inv_qq;  // 2^32, 2^-32, 2^-44
  double band0;      // the part of fx_pca's "near" band that does not depend on the cluster: 1e-14 + 3 B_cov, this path's own grids (see fx_pca)
  uint32_t *rkey;          // root hash: key + 1 (0 = empty); the slot is the index of the root's block
  uint32_t *rlist;         // [kFxSub * mr_per] slots of the roots created in this sweep, per sub-counter
  uint32_t tr_mask;
  uint32_t static_map;  // k_fx_nodes: static hand-out of the parents (small sweeps), see there
  unsigned long long *blk;   // [tr_mask + 1][kFxBlockW]
  unsigned long long *blk2;  // [kFxSub * mq_per][kFxBlockW]
  unsigned long long *rec;   // [2][rec_cap][kFxRecW]: records of the layer-0/1 pass | of the layer-2 pass
  uint32_t rec_tiles;        // records [0, rec_tiles * kFxRecTile) belong to the tiles, the rest is the spill pool
  uint32_t spill_per;        // records per spill sub-pool (eight of them)
  uint32_t rec_cap;
  uint32_t mr_per, mq_per;
  uint32_t fmt;  // layout of the points: 0 any strides, 1 the reference's 48-byte records (16-byte aligned), 2 packed 12 + 8 bytes (16-byte aligned)
  uint32_t *status;
  uint32_t *cnt;            // [4 banks][kFxSub] sub-counters, kFxCntStride words apart
  unsigned long long *jobs;  // [grid of k_fx_nodes][kFxJobCap][kFxJobW]: closed temporal clusters waiting for their node's test
  // the two-kernel form of the node stage (extract_split.inc: large clouds, batches of sweeps)
  unsigned long long *nodes;     // [wave of eight parents][kFxNodeW][64 lanes]: totals + cluster count of every child node
  uint32_t *wdesc;               // [wave of eight parents][64 words]: parents, root cluster counts, the wave's jobs
  unsigned long long *jobpool;   // [8 sub-pools][jobpool_per][kFxJobW]
  uint32_t jobpool_per;
  // emission (shared with the exact path)
  wc_surfel *slots;
  wc_surfel_id *slot_ids;
  uint32_t slots_per;       // slots per sub-range
  uint32_t *slot_counts;
  uint64_t *slot_bins;
  uint32_t slot_bin_cap;
};

// `why` (0..23) names the call site for wc_debug_status (word 32 + why of the host mailbox): which rule sent a sweep to the exact path
__device__ __forceinline__ void fx_fallback(uint32_t *status, int why) {
  raise_flag(status, kFlagFxFallback);
  uint32_t *hm = host_mailbox(status);
  if (hm) hm[32 + why] = 1u;
}
__device__ __forceinline__ uint32_t *fx_cnt(const FxArgs &A, uint32_t bank, uint32_t j) { return A.cnt + (bank * kFxSub + j) * kFxCntStride; }

__device__ __forceinline__ uint32_t fx_hash32(uint32_t k) {
  k ^= k >> 16;
  k *= 0x7FEB352Du;
  k ^= k >> 15;
  k *= 0x846CA68Bu;
  k ^= k >> 16;
  return k;
}

// VoxelLoc (surfel_extraction.h:59-64) = floor(fl(p / vs)): p * (1 / vs) decides except within 1e-9 of an integer, where the
// true fp64 division is repeated (the rounded quotient may sit on the other side of the integer)
// (FINITE p only: the conversions are bare.  Pass A calls it for finite points alone, and a non-finite origin is replaced before its
// index is used; a finite quotient beyond int32 saturates here where vox() gives INT32_MIN - kFlagKeyRange either way)
__device__ __forceinline__ int fx_vox(double p, double vs, double inv_vs) {
  const double q = p * inv_vs;
  const double r = rint(q);
  if (fabs(q - r) > 1e-9 * (fabs(r) + 1.0)) return (int)floor(q);
  return (int)floor(p / vs);
}

// slot of a root voxel in the insert-only hash (the slot IS the index of the root's block), or ~0 (lookup of an absent key /
// table full: the flag is raised).  The lane that creates the root appends the slot to the dense root list k_fx_nodes walks.
// Status word kFxStMaxProbe: the largest displacement of a root from its home slot in this sweep.  k_fx_nodes<1> CLEARS the entries of
// the roots that queued nothing for layer 2, so a lookup in k_fx_acc<2> may meet an empty slot in front of a displaced root that is
// still there: it only stops at an empty slot beyond that displacement.  (Rounds 2 - 4 stopped at the first empty slot: two roots
// with one home slot, the one that inserted second keeping layer-2 nodes, the first one cleared -> the second root's points were
// silently skipped by the layer-2 pass and a layer-2 surfel could go missing, depending on which tile inserted first.  Found in
// round 5 by a parameter test at voxel size 0.95, one run in three.)
constexpr int kFxStMaxProbe = 20;
__device__ __forceinline__ uint32_t fx_root_slot(const FxArgs &A, uint32_t key1, uint32_t sub, bool insert, uint32_t maxprobe = 0u) {
  uint32_t slot = fx_hash32(key1) & A.tr_mask;
  for (int probe = 0; probe < 64; ++probe) {
    uint32_t k;
    if (insert) {
      k = atomicCAS(&A.rkey[slot], 0u, key1);
      if (k == 0u) {
        if (probe) atomicMax(&A.status[kFxStMaxProbe], (uint32_t)probe);
        const uint32_t local = atomicAdd(fx_cnt(A, kFxStRoots, sub), 1u);
        if (local < A.mr_per)
          A.rlist[sub * A.mr_per + local] = slot;
        else
          fx_fallback(A.status, 0);
        return slot;
      }
    } else {
      k = __hip_atomic_load(&A.rkey[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k == 0u && (uint32_t)probe >= maxprobe) return 0xFFFFFFFFu;
    }
    if (k == key1) return slot;
    slot = (slot + 1u) & A.tr_mask;
  }
  fx_fallback(A.status, 1);
  return 0xFFFFFFFFu;
}

struct FxPart {  // integer moments of a stretch of points of one cell
  uint32_t n;
  long long st, s[3], ss[6];
  unsigned long long tmin_inv, tmax_p1;  // max of (kFxTMax - tick), max of (tick + 1): both grow by (atomic) max from zero
};
__device__ __forceinline__ void fx_zero(FxPart &a) {
  a.n = 0, a.st = 0, a.tmin_inv = 0, a.tmax_p1 = 0;
  for (int i = 0; i < 3; ++i) a.s[i] = 0;
  for (int i = 0; i < 6; ++i) a.ss[i] = 0;
}
__device__ __forceinline__ void fx_acc(FxPart &a, const FxPart &b) {
  a.n += b.n, a.st += b.st;
  for (int i = 0; i < 3; ++i) a.s[i] += b.s[i];
  for (int i = 0; i < 6; ++i) a.ss[i] += b.ss[i];
  a.tmin_inv = max(a.tmin_inv, b.tmin_inv);
  a.tmax_p1 = max(a.tmax_p1, b.tmax_p1);
}

// adds a partial to a cell of the tile's LDS hash (13 words) with ds atomics
__device__ __forceinline__ void fx_add_cell(unsigned long long *cell, const FxPart &a) {
  atomicAdd((uint32_t *)cell, a.n);
  atomicAdd(&cell[1], (unsigned long long)a.st);
  for (int i = 0; i < 3; ++i) atomicAdd(&cell[2 + i], (unsigned long long)a.s[i]);
  for (int i = 0; i < 6; ++i) atomicAdd(&cell[5 + i], (unsigned long long)a.ss[i]);
  atomicMax(&cell[11], a.tmin_inv);
  atomicMax(&cell[12], a.tmax_p1);
}

// One cell of one tile -> one record in HBM, pushed onto the list of its (node, time slot) with one atomic exchange.
// LEVEL 1: code = root key (30) | o1 << 30 | bin << 33; LEVEL 2: node (28) | o2 << 28 | bin << 31.  ridx = record index.
// WAVE-UNIFORM call (lanes without a record pass active = false): the lanes of a wavefront mostly push cells of the same few
// root voxels, and same-address atomics of one instruction are expensive - one lane per distinct root does the hash insert
// and the header update for all of them.
// A push has THREE steps, which k_fx_acc may issue apart (its form bit 1: link early, store late):
//   fx_link_claim  the wavefront's distinct parents, a leader lane and the smallest bin of each; every leader issues the first probe
//                  of its root's hash insert (LEVEL 1)
//   fx_link_head   the leaders finish the claim (further probes are rare), append the roots they created to the dense root list and
//                  raise the header's smallest bin; every lane exchanges its list head for ridx + 1 and gets `old`
//   fx_store       the record's fourteen words, `old` among them
// The link needs the cell code and the record index alone, not the sums: issued as soon as the codes are known, its atomics' round
// trips run beside pass B and the cross-lane merge.  Nothing reads a list inside k_fx_acc, so a head may name a record that is
// written later in the same kernel; k_fx_nodes starts behind the kernel boundary.
struct FxClaim {  // per lane: the leader lane of the lane's parent, the parent's smallest bin, the home slot and what the leader's probe found there
  int lead;
  uint32_t gmb, s0, found;
};
template <int LEVEL>
__device__ __forceinline__ void fx_code_fields(unsigned long long code, uint32_t &pkey, uint32_t &oct, uint32_t &bin) {
  if (LEVEL == 1) {
    pkey = (uint32_t)(code & 0x3FFFFFFFull) + 1u;
    oct = (uint32_t)(code >> 30) & 7u;
    bin = (uint32_t)(code >> 33) & 0xFFFFFu;
  } else {
    pkey = (uint32_t)(code & 0xFFFFFFFull) + 1u;
    oct = (uint32_t)(code >> 28) & 7u;
    bin = (uint32_t)(code >> 31) & 0xFFFFFu;
  }
}
template <int LEVEL>
__device__ __forceinline__ FxClaim fx_link_claim(const FxArgs &A, bool active, unsigned long long code) {
  const int lane = threadIdx.x & 63;
  uint32_t oct, bin, pkey;
  fx_code_fields<LEVEL>(code, pkey, oct, bin);
  // the distinct parents of the wavefront: leader lane and smallest bin of each (registers only)
  int lead = lane;
  uint32_t gmb = bin;
  {
    unsigned long long todo = __ballot(active);
    while (todo) {
      const int first = __ffsll((long long)todo) - 1;
      const uint32_t k0 = (uint32_t)__shfl((int)pkey, first);
      const bool mine = active && pkey == k0;
      uint32_t mb = mine ? bin : 0xFFFFFFFFu;
      for (int m = 1; m < 64; m <<= 1) mb = min(mb, (uint32_t)__shfl_xor((int)mb, m));
      if (mine) lead = first, gmb = mb;
      todo &= ~__ballot(mine);
    }
  }
  // every leader claims / finds its parent's block AT THE SAME TIME (one round trip for the wavefront's parents, not one
  // per parent); the roots created here are appended to the dense root list with one counter atomic per wavefront, whose
  // answer is only awaited after the list heads have been exchanged
  FxClaim c;
  c.lead = lead, c.gmb = gmb, c.s0 = 0u, c.found = 0u;
  if (LEVEL == 1) {
    c.s0 = fx_hash32(pkey) & A.tr_mask;
    if (active && lane == lead && !(WC_DBG(A.P, 64))) c.found = atomicCAS(&A.rkey[c.s0], 0u, pkey);
  }
  return c;
}
// returns whether the lane's record is to be written; old: the list's previous head (the record's word 13)
template <int LEVEL>
__device__ __forceinline__ bool fx_link_head(const FxArgs &A, bool active, unsigned long long code, uint32_t sub, uint32_t ridx, const FxClaim &c,
                                             uint32_t &old) {
  const int lane = threadIdx.x & 63;
  unsigned long long *blk = nullptr;
  uint32_t oct, bin, pkey;
  fx_code_fields<LEVEL>(code, pkey, oct, bin);
  const int lead = c.lead;
  const uint32_t gmb = c.gmb;
  const bool leader = active && lane == lead;
  uint32_t slot = 0xFFFFFFFFu;
  bool created = false;
  if (leader) {
    if (LEVEL == 1) {
      if (WC_DBG(A.P, 64)) {
        slot = c.s0;
      } else if (c.found == 0u || c.found == pkey) {
        slot = c.s0;
        created = c.found == 0u;
      } else {
        uint32_t s = (c.s0 + 1u) & A.tr_mask;
        for (int probe = 1; probe < 64; ++probe) {
          const uint32_t k = atomicCAS(&A.rkey[s], 0u, pkey);
          if (k == 0u || k == pkey) {
            slot = s;
            created = k == 0u;
            if (created && probe) atomicMax(&A.status[kFxStMaxProbe], (uint32_t)probe);  // (a displaced root: see fx_root_slot)
            break;
          }
          s = (s + 1u) & A.tr_mask;
        }
        if (slot == 0xFFFFFFFFu) fx_fallback(A.status, 2);
      }
    } else {
      slot = pkey - 1u;
    }
  }
  const unsigned long long cm = __ballot(created);
  uint32_t list_base = 0;
  const int cfirst = cm ? __ffsll((long long)cm) - 1 : 0;
  if (cm && lane == cfirst) list_base = atomicAdd(fx_cnt(A, kFxStRoots, sub), (uint32_t)__popcll(cm));
  if (leader && slot != 0xFFFFFFFFu && !(WC_DBG(A.P, 8))) {
    unsigned long long *b0 = (LEVEL == 1 ? A.blk : A.blk2) + (size_t)slot * kFxBlockW;
    atomicMax((uint32_t *)b0 + 2, 0xFFFFFFFFu - gmb);  // smallest bin of the block
  }
  const uint32_t myslot = (uint32_t)__shfl((int)slot, lead);
  old = 0u;
  const bool ok = active && myslot != 0xFFFFFFFFu;
  if (ok) {
    blk = (LEVEL == 1 ? A.blk : A.blk2) + (size_t)myslot * kFxBlockW;
    uint32_t *heads = (uint32_t *)(blk + kFxHdrW);
    if (!(WC_DBG(A.P, 32))) old = atomicExch(&heads[oct * kFxSlots + (bin & (kFxSlots - 1))], ridx + 1u);
  }
  if (cm) {
    list_base = (uint32_t)__shfl((int)list_base, cfirst);
    if (created) {
      const uint32_t local = list_base + (uint32_t)__popcll(cm & ((1ull << lane) - 1ull));
      if (local < A.mr_per)
        A.rlist[sub * A.mr_per + local] = slot;
      else
        fx_fallback(A.status, 3);
    }
  }
  return ok;
}
// (called by the lanes whose record is to be written only)
template <int LEVEL>
__device__ __forceinline__ void fx_store(const FxArgs &A, unsigned long long code, const FxPart &a, uint32_t ridx, uint32_t old) {
  if (WC_DBG(A.P, 16)) return;
  uint32_t oct, bin, pkey;
  fx_code_fields<LEVEL>(code, pkey, oct, bin);
  unsigned long long *rec = A.rec + ((size_t)(LEVEL - 1) * A.rec_cap + ridx) * kFxRecW;
  ulonglong2 *r2 = (ulonglong2 *)rec;
  r2[0] = make_ulonglong2((unsigned long long)a.n | ((unsigned long long)bin << 32), (unsigned long long)a.st);
  r2[1] = make_ulonglong2((unsigned long long)a.s[0], (unsigned long long)a.s[1]);
  r2[2] = make_ulonglong2((unsigned long long)a.s[2], (unsigned long long)a.ss[0]);
  r2[3] = make_ulonglong2((unsigned long long)a.ss[1], (unsigned long long)a.ss[2]);
  r2[4] = make_ulonglong2((unsigned long long)a.ss[3], (unsigned long long)a.ss[4]);
  r2[5] = make_ulonglong2((unsigned long long)a.ss[5], a.tmin_inv);
  r2[6] = make_ulonglong2(a.tmax_p1, (unsigned long long)old);  // next record of this (node, slot) list, 0 = end
}
// the three steps in one place (WAVE-UNIFORM call): the tile's hash cells, the spill pool, and the direct records of a form that
// links where it stores
template <int LEVEL>
__device__ __forceinline__ void fx_push(const FxArgs &A, bool active, unsigned long long code, const FxPart &a, uint32_t sub, uint32_t ridx) {
  const FxClaim c = fx_link_claim<LEVEL>(A, active, code);
  uint32_t old;
  if (fx_link_head<LEVEL>(A, active, code, sub, ridx, c, old)) fx_store<LEVEL>(A, code, a, ridx, old);
}

// ---- pass A for ONE point: every form of k_fx_acc forms a point's cell code and integer coordinates with these routines ----------
struct FxPt {
  unsigned long long code;  // 0: the point is skipped
  double tmag;              // fma(t - t_lo, 2^s, M): the tick in magic form
  uint32_t qlx, qly, qlz;   // low words of fma(p - cc, 2^32, M): the high word is M's (|q| < 2^31)
};
// voxel index floor(p (1 / vs)); returns whether the point is finite.  The rare coordinate within 1e-6 of a voxel face is divided
// properly (fx_vox) in a WAVE-UNIFORM block: the fractional part against an ABSOLUTE 1e-6 is wider than fx_vox's own relative band up
// to |q| ~ 1000, and p (1 / vs) is within 5e-16 |q| of p / vs, i.e. inside the band for every coordinate a float can resolve to a
// voxel - two compares on a value the floor needs anyway instead of rint + a relative bound.  A non-finite coordinate fails the face
// test (q - floor(q) is NaN for NaN and for +-inf), so the finite-point rule is looked at in the rare block alone and the common path
// pays nothing for it.
__device__ __forceinline__ bool fx_pt_index(const FxArgs &A, double x, double y, double z, int &kx, int &ky, int &kz) {
  const double qx = x * A.inv_vs, qy = y * A.inv_vs, qz = z * A.inv_vs;
  const double fx = floor(qx), fy = floor(qy), fz = floor(qz);
  const double dx = qx - fx, dy = qy - fy, dz = qz - fz;
  const bool near = !(dx > 1e-6 && dx < 1.0 - 1e-6) || !(dy > 1e-6 && dy < 1.0 - 1e-6) || !(dz > 1e-6 && dz < 1.0 - 1e-6);
  kx = (int)fx, ky = (int)fy, kz = (int)fz;
  bool fin = true;
  if (__ballot(near)) {
    fin = finite3(x, y, z);  // (a non-finite point needs no index)
    if (__ballot(fin && near)) {
      if (fin) kx = fx_vox(x, A.P.vs, A.inv_vs), ky = fx_vox(y, A.P.vs, A.inv_vs), kz = fx_vox(z, A.P.vs, A.inv_vs);
    }
  }
  return fin;
}
// key of the root voxel relative to the origin voxel k0 (10 bits per axis)
__device__ __forceinline__ bool fx_pt_key(int kx, int ky, int kz, int k0x, int k0y, int k0z, uint32_t &key) {
  const int rx = kx - k0x + 512, ry = ky - k0y + 512, rz = kz - k0z + 512;
  key = (uint32_t)rx | ((uint32_t)ry << 10) | ((uint32_t)rz << 20);
  return (unsigned)rx < 1024u && (unsigned)ry < 1024u && (unsigned)rz < 1024u;
}
// octant, tick, time bin, cell code and the magic-form coordinates.  have: the point exists and is finite.  LEVEL 2: split / base2 are
// the queued layer-1 nodes of the point's root and where their blocks start.  No early exit: the range flags are raised by the caller,
// once (with the checks as exits the compiler ran the four chains of a lane one after the other).
// Integer moments from fp64 instructions (round 5).  With M = 1.5 x 2^52, fma(a, 2^32, M) holds rint(a 2^32) in the low mantissa
// bits of a double whose exponent is fixed: its BIT PATTERN minus M's is that integer.  So a coordinate q (units of 2^-32 m, |q| <
// 2^31), a tick (< 2^41) and - with M2 = 1.5 x 2^72 - a product q_i q_j rounded to the 2^20 grid (units of 2^-64 m^2: the 2^-44 m^2
// of the records) are each ONE fma, and their exact sums are 64-bit integer additions of the bit patterns: n x bits(M) is taken off
// the high words when a partial closes (fx_fix).
template <int LEVEL>
__device__ __forceinline__ FxPt fx_pt_code(const FxArgs &A, bool have, double x, double y, double z, double t, int kx, int ky, int kz, int k0x,
                                           int k0y, int k0z, uint32_t split, uint32_t base2, bool &bad_key, bool &bad_time) {
  const ExParams &P = A.P;
  uint32_t key;
  const bool key_ok = fx_pt_key(kx, ky, kz, k0x, k0y, k0z, key);
  // octants exactly as CutOctoTree forms them (cc:147-165): strict >, child centre = centre +- quarter in float
  // (0.5 + k) vs is exact in fp64 (the voxel size is a float - 24 significant bits - and 0.5 + k a handful), so is the fused form
  // k vs + vs / 2: the same value, one instruction less per axis
  const double cx = fma((double)kx, (double)P.vs_f, 0.5 * (double)P.vs_f), cy = fma((double)ky, (double)P.vs_f, 0.5 * (double)P.vs_f),
               cz = fma((double)kz, (double)P.vs_f, 0.5 * (double)P.vs_f);
  const int bx = x > cx, by = y > cy, bz = z > cz;
  const uint32_t o1 = (uint32_t)(4 * bx + 2 * by + bz);
  // time: tick = (t - t_lo) 2^s (exact for stamps on a 2^-s grid), bin = floor((t - t_lo) / w)
  const double trel = t - A.t_lo;
  const double tm = fma(trel, A.tick, kFxMagic);  // (tick = 2^s: the product is exact, the fma rounds it to an integer once)
  const bool time_ok = tm >= kFxMagic && tm < kFxMagic + 2199023255552.0;  // tick in [0, 2^41)
  bad_key = bad_key || (have && !key_ok);
  bad_time = bad_time || (have && key_ok && !time_ok);
  bool use = have && key_ok && time_ok;
  const uint32_t bin = (uint32_t)(use ? trel * A.inv_w : 0.0);
  unsigned long long c;
  if (LEVEL == 1) {
    c = (unsigned long long)key | ((unsigned long long)o1 << 30) | ((unsigned long long)bin << 33) | (1ull << 63);
  } else {
    const float q0 = P.vs_f / 4;
    use = use && ((split >> o1) & 1u);
    const uint32_t qn = base2 + (uint32_t)__popc(split & ((1u << o1) - 1u));
    const double c1x = cx + (double)((float)(2 * bx - 1) * q0), c1y = cy + (double)((float)(2 * by - 1) * q0),
                 c1z = cz + (double)((float)(2 * bz - 1) * q0);
    const uint32_t o2 = (uint32_t)(4 * (x > c1x) + 2 * (y > c1y) + (z > c1z));
    c = (unsigned long long)qn | ((unsigned long long)o2 << 28) | ((unsigned long long)bin << 31) | (1ull << 63);
  }
  // coordinates relative to the voxel centre ITSELF: (0.5 + k) vs is exact (above), a multiple of 2^-25 m for a voxel size in
  // [0.5, 1); p is a float widened, so p - centre is exact as well and (p - centre) 2^32 an integer for |p| >= 2^-8 m (the fma rounds
  // the rest)
  FxPt o;
  o.code = use ? c : 0ull;
  o.tmag = tm;
  const double mx = fma(x - cx, A.qs, kFxMagic), my = fma(y - cy, A.qs, kFxMagic), mz = fma(z - cz, A.qs, kFxMagic);
  // (the mantissa is 2^51 + q: its low word is q mod 2^32, its high word M's for q >= 0 and M's - 1 for q < 0 - pass B rebuilds the
  // double from the low word alone; points with code 0 are skipped there: whatever these hold)
  o.qlx = (uint32_t)__double_as_longlong(mx), o.qly = (uint32_t)__double_as_longlong(my), o.qlz = (uint32_t)__double_as_longlong(mz);
  return o;
}
// the whole of pass A for one point of the layer-0/1 pass.  in_range: the point's index is below the sweep's point count
__device__ __forceinline__ FxPt fx_point(const FxArgs &A, bool in_range, double x, double y, double z, double t, int k0x, int k0y, int k0z,
                                         bool &bad_key, bool &bad_time) {
  int kx, ky, kz;
  const bool fin = fx_pt_index(A, x, y, z, kx, ky, kz);
  return fx_pt_code<1>(A, in_range && fin, x, y, z, t, kx, ky, kz, k0x, k0y, k0z, 0u, 0u, bad_key, bad_time);
}

// ---- the streaming pass ---------------------------------------------------------------------------------------------------
// the raw values of a tile as its threads fetch them (lane = point, four rounds): held in registers between the request and the
// LDS transposition, so that a persistent workgroup can request tile i + 1 before it works on tile i
struct FxRaw {
  float x[kFxPts], y[kFxPts], z[kFxPts];
  double t[kFxPts];
};
// FULL: the tile lies inside the sweep (a wave-uniform test of the caller's) - its loads are unconditional, so that whoever uses the
// rounds one after the other waits for a COUNT of outstanding loads, not for all of them (a branch around a load drains the counter)
template <bool FULL = false>
__device__ __forceinline__ FxRaw fx_acc_load(const FxArgs &A, const uint32_t bid) {
  FxRaw r;
  const uint64_t tb = (uint64_t)bid * kFxTile, n = A.pts.n;
#pragma unroll
  for (int it = 0; it < kFxPts; ++it) {
    const uint64_t i = tb + (uint64_t)it * kFxThreads + threadIdx.x;
    r.x[it] = r.y[it] = r.z[it] = 0.f, r.t[it] = 0.0;
    if (FULL || i < n) {
      // (Round 5 tried ONE 16-byte load for x, y, z, pad of a 48-byte record + the stamp at +24 - two requests per point instead of
      // four: k_fx_acc<1> 19.7 - 21.2 -> 21.5 - 23 us at C2, alternating builds on one box.  Element-wise loads stay.)
      const float *f = (const float *)((const char *)A.pts.xyz + i * A.pts.xyz_stride);
      r.x[it] = f[0], r.y[it] = f[1], r.z[it] = f[2];
      r.t[it] = load_t(A.pts, i);
    }
    // (issue order = round order: the scheduler otherwise moves the stamps' loads behind the coordinates' and round 0 waits for round 3's)
    if (FULL) __builtin_amdgcn_sched_barrier(0);
  }
  return r;
}

// FORM (development option fx_acc_form; kFxAccForm is what the library runs): bit 0 - LEVEL 1, staged path: pass A per load round,
// under the loads; bit 1 - the direct records are linked as soon as the codes are known and stored where the sums exist.  0 is the
// order of rounds 2 - 6 - all loads, transposition, pass A, pass B, link + store - WITHOUT round 5's early first hash probe (FxEarly,
// which bit 1 replaced): nothing of the link goes out before the sums exist, so form 0 is slower than the kernel of round 6.  Every form writes the same bytes.
constexpr int kFxAccForm = 3;
template <int LEVEL, int FORM>
__device__ __forceinline__ void fx_acc_body(const FxArgs &A, const uint32_t bid) {  // bid: this workgroup's tile of ITS sweep
  constexpr bool kRounds = LEVEL == 1 && (FORM & 1) != 0, kLinkEarly = (FORM & 2) != 0;
  // LDS: first the staging area of the tile's points (20 KB of raw values, or 28 KB of pass A's results where pass A runs per load
  // round), then - the points are in registers - the tile's cell hash (28 KB) in the same bytes: 28 KB per workgroup = five
  // workgroups per CU, the whole grid of a 1 M-point sweep resident
  __shared__ unsigned long long lds_raw[kFxLds * 14];
  unsigned long long *h_key = lds_raw;                                        // [kFxLds]
  unsigned long long(*h_rec)[13] = (unsigned long long(*)[13])(lds_raw + kFxLds);  // [kFxLds][13]
  static_assert(kFxLds * 14 * 8 >= kFxTile * 20, "staging area fits the hash area");
  const int tid = threadIdx.x;
  const ExParams &P = A.P;
  const uint32_t sub = bid & (kFxSub - 1);
  const uint64_t n = A.pts.n;
  const uint64_t base = ((uint64_t)bid * kFxThreads + tid) * kFxPts;
  static_assert(kFxPts == 4, "the LDS transposition reads four points per lane");
  const bool full = ((uint64_t)bid + 1u) * kFxTile <= n;  // wave-uniform
  const bool direct = A.fmt == 2u && full;
  // ---- pass A: cell code, time tick and integer coordinates of the lane's four points (code 0: the point is skipped): fx_point ----
  unsigned long long code[kFxPts];
  double tmag[kFxPts];
  uint32_t qlx[kFxPts], qly[kFxPts], qlz[kFxPts];
  bool bad_key = false, bad_time = false;
  if (kRounds && !direct) {
    // PASS A PER LOAD ROUND.  Pass A needs one point at a time, not the lane-owns-four-consecutive-points layout of pass B and the
    // scan: the loads stay lane = point in four rounds, all issued at once, and the lane runs fx_point on round r's point as soon as
    // round r has returned - the SIMDs work while the memory system serves the later rounds.  The RESULTS (28 bytes per point: code,
    // tick, three low words; struct of arrays) are transposed through LDS instead of the raw values (20 bytes): exactly the bytes of
    // the cell hash, which takes them over behind the same barriers as before.
    static_assert(kFxTile * 28 == kFxLds * 14 * 8, "the staged results fill the hash area exactly");
    unsigned long long *s_code = lds_raw;                    // [kFxTile]
    double *s_tm = (double *)(lds_raw + kFxTile);          // [kFxTile]
    uint32_t *s_qx = (uint32_t *)(lds_raw + 2 * kFxTile), *s_qy = s_qx + kFxTile, *s_qz = s_qy + kFxTile;
    // the key origin's load goes out in front of the tile's: its voxel is needed before round 0
    double x0, y0, z0;
    load_xyz(A.pts, 0, x0, y0, z0);
    // (one copy of the rounds per kind of tile: joined in front of the rounds, the full tile's registers would meet the partial
    // tile's guarded ones and the compiler waits for the loads where it merges them)
    auto rounds = [&](auto full_tag) -> bool {
      constexpr bool kFull = decltype(full_tag)::value;
      const FxRaw raw = fx_acc_load<kFull>(A, bid);
      if (!finite3(x0, y0, z0)) ex_origin(A.pts, x0, y0, z0);  // (wave-uniform, rare)
      const int k0x = fx_vox(x0, P.vs, A.inv_vs), k0y = fx_vox(y0, P.vs, A.inv_vs), k0z = fx_vox(z0, P.vs, A.inv_vs);
      if (WC_DBG(P, 4)) {  // profiling experiment: loads only
        double sacc = 0;
#pragma unroll
        for (int j = 0; j < kFxPts; ++j) sacc += (double)raw.x[j] + (double)raw.y[j] + (double)raw.z[j] + raw.t[j];
        if (sacc == 1.2345) h_key[tid] = 1ull;
        return false;
      }
      const uint64_t tb = (uint64_t)bid * kFxTile;
#pragma unroll
      for (int it = 0; it < kFxPts; ++it) {
        const uint32_t i = (uint32_t)it * kFxThreads + (uint32_t)tid;
        const FxPt p = fx_point(A, kFull || tb + i < n, (double)raw.x[it], (double)raw.y[it], (double)raw.z[it], raw.t[it], k0x, k0y, k0z, bad_key,
                                bad_time);
        s_code[i] = p.code, s_tm[i] = p.tmag;
        s_qx[i] = p.qlx, s_qy[i] = p.qly, s_qz[i] = p.qlz;
      }
      return true;
    };
    if (!(full ? rounds(std::true_type{}) : rounds(std::false_type{}))) return;
    __syncthreads();
    {  // the lane's four consecutive points: 16-byte LDS reads
      const ulonglong2 c01 = ((const ulonglong2 *)s_code)[2 * tid], c23 = ((const ulonglong2 *)s_code)[2 * tid + 1];
      const double2 t01 = ((const double2 *)s_tm)[2 * tid], t23 = ((const double2 *)s_tm)[2 * tid + 1];
      const uint4 vx = ((const uint4 *)s_qx)[tid], vy = ((const uint4 *)s_qy)[tid], vz = ((const uint4 *)s_qz)[tid];
      code[0] = c01.x, code[1] = c01.y, code[2] = c23.x, code[3] = c23.y;
      tmag[0] = t01.x, tmag[1] = t01.y, tmag[2] = t23.x, tmag[3] = t23.y;
      qlx[0] = vx.x, qlx[1] = vx.y, qlx[2] = vx.z, qlx[3] = vx.w;
      qly[0] = vy.x, qly[1] = vy.y, qly[2] = vy.z, qly[3] = vy.w;
      qlz[0] = vz.x, qlz[1] = vz.y, qlz[2] = vz.z, qlz[3] = vz.w;
    }
    __syncthreads();  // every lane has its points: the staging bytes become the (empty) cell hash
    for (int i = tid; i < kFxLds * 14; i += kFxThreads) lds_raw[i] = 0ull;
    __syncthreads();
  } else {
  // the order of rounds 2 - 6 (LEVEL 2: its per-point hash look-ups are loads of their own and would drain the tile's in order; packed
  // points: no staging at all).  The tile's loads go out FIRST (in front of point 0's and the divisions behind it)
  FxRaw raw;
  float4 da = make_float4(0.f, 0.f, 0.f, 0.f), db = da, dc = da;
  double2 dt01 = make_double2(0.0, 0.0), dt23 = dt01;
  if (direct) {
    const float4 *xp = (const float4 *)((const char *)A.pts.xyz + base * 12u);
    const double2 *tp = (const double2 *)((const char *)A.pts.time + base * 8u);
    da = xp[0], db = xp[1], dc = xp[2];
    dt01 = tp[0], dt23 = tp[1];
  } else {
    raw = fx_acc_load(A, bid);
  }
  double x0, y0, z0;
  load_xyz(A.pts, 0, x0, y0, z0);  // (the key origin, if it is finite: looked at behind pass A's voxel indices, where ex_origin() replaces a non-finite one)
  // (fx_vox = floor(p / vs) by construction - the product with 1 / vs decides unless it lies within 1e-9 of an integer - without the
  // three divisions of vox(), ~35 instructions of every wavefront for a value all wavefronts share)
  int k0x = fx_vox(x0, P.vs, A.inv_vs), k0y = fx_vox(y0, P.vs, A.inv_vs), k0z = fx_vox(z0, P.vs, A.inv_vs);

  // the tile's points: coalesced loads (lane = point, four rounds: fx_acc_load) into LDS, then every lane takes FOUR CONSECUTIVE
  // points (a lane that reads its own 4 x 48 bytes straight from HBM runs at half the rate: 64 scattered 12-byte pieces per
  // load instruction)
  double px[kFxPts], py[kFxPts], pz[kFxPts], pt[kFxPts];
  if (direct) {
    // packed points (what wc_undistort_sweep_packed writes): the lane's four consecutive points are 48 + 32 CONTIGUOUS bytes - five
    // 16-byte loads per lane, each instruction covering every byte of the lines it touches over the three (two) of them; no staging
    // in LDS, no transposition, two barriers less.  (The 48-byte records stay on the staged path: a lane reading its own 4 x 48 bytes
    // fetches 64 scattered 16-byte pieces per instruction - half the rate, measured in round 2.)
    const float4 a = da, b = db, c = dc;
    const double2 t01 = dt01, t23 = dt23;
    for (int i = tid; i < kFxLds * 14; i += kFxThreads) lds_raw[i] = 0ull;  // (the empty cell hash, while the loads are under way)
    px[0] = a.x, py[0] = a.y, pz[0] = a.z, px[1] = a.w, py[1] = b.x, pz[1] = b.y;
    px[2] = b.z, py[2] = b.w, pz[2] = c.x, px[3] = c.y, py[3] = c.z, pz[3] = c.w;
    pt[0] = t01.x, pt[1] = t01.y, pt[2] = t23.x, pt[3] = t23.y;
    __syncthreads();
  } else {
    double *s_t = (double *)lds_raw;                 // [kFxTile]
    float *s_x = (float *)(s_t + kFxTile), *s_y = s_x + kFxTile, *s_z = s_y + kFxTile;
#pragma unroll
    for (int it = 0; it < kFxPts; ++it) {
      s_x[it * kFxThreads + tid] = raw.x[it], s_y[it * kFxThreads + tid] = raw.y[it], s_z[it * kFxThreads + tid] = raw.z[it];
      s_t[it * kFxThreads + tid] = raw.t[it];
    }
    __syncthreads();
    {
      const float4 vx = ((const float4 *)s_x)[tid], vy = ((const float4 *)s_y)[tid], vz = ((const float4 *)s_z)[tid];
      const double2 t01 = ((const double2 *)s_t)[2 * tid], t23 = ((const double2 *)s_t)[2 * tid + 1];
      px[0] = vx.x, px[1] = vx.y, px[2] = vx.z, px[3] = vx.w;
      py[0] = vy.x, py[1] = vy.y, py[2] = vy.z, py[3] = vy.w;
      pz[0] = vz.x, pz[1] = vz.y, pz[2] = vz.z, pz[3] = vz.w;
      pt[0] = t01.x, pt[1] = t01.y, pt[2] = t23.x, pt[3] = t23.y;
    }
    __syncthreads();  // every lane has its points: the staging bytes become the (empty) cell hash
    for (int i = tid; i < kFxLds * 14; i += kFxThreads) lds_raw[i] = 0ull;
    __syncthreads();
  }
  if (WC_DBG(P, 4)) {  // profiling experiment: loads only
    double sacc = 0;
#pragma unroll
    for (int j = 0; j < kFxPts; ++j) sacc += px[j] + py[j] + pz[j] + pt[j];
    if (sacc == 1.2345) h_key[tid] = 1ull;
    return;
  }
  // voxel indices first (the four chains of a lane side by side), then - LEVEL 2 - the look-ups, then the codes
  int kxs[kFxPts], kys[kFxPts], kzs[kFxPts];
  bool fin[kFxPts];
#pragma unroll
  for (int j = 0; j < kFxPts; ++j) fin[j] = fx_pt_index(A, px[j], py[j], pz[j], kxs[j], kys[j], kzs[j]);
  if (!finite3(x0, y0, z0)) {  // (wave-uniform; here, behind the tile's loads, not in front of them)
    ex_origin(A.pts, x0, y0, z0);
    k0x = fx_vox(x0, P.vs, A.inv_vs), k0y = fx_vox(y0, P.vs, A.inv_vs), k0z = fx_vox(z0, P.vs, A.inv_vs);
  }
  // LEVEL 2: which layer-1 nodes of each point's root were queued, and where their blocks start - the four roots of a lane
  // looked up TOGETHER (hash probe, then the root's header: two round trips for the lane; one root after the other - a sweep in
  // firing order has four different ones - was up to eight, and most of this launch)
  uint32_t split4[kFxPts], base4[kFxPts];
#pragma unroll
  for (int j = 0; j < kFxPts; ++j) split4[j] = base4[j] = 0u;
  if (LEVEL == 2) {
    uint32_t key1[kFxPts], slot4[kFxPts], found4[kFxPts];
    bool ok4[kFxPts];
#pragma unroll
    for (int j = 0; j < kFxPts; ++j) {
      uint32_t key;
      const bool key_ok = fx_pt_key(kxs[j], kys[j], kzs[j], k0x, k0y, k0z, key);
      ok4[j] = base + j < n && fin[j] && key_ok;
      key1[j] = key + 1u;
      slot4[j] = fx_hash32(key1[j]) & A.tr_mask;
    }
#pragma unroll
    for (int j = 0; j < kFxPts; ++j) found4[j] = ok4[j] ? __hip_atomic_load(&A.rkey[slot4[j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    // (another key in the home slot - or an EMPTY home slot in a sweep that displaced roots: the slot's root may have been cleared by
    // k_fx_nodes<1> while a displaced root behind it is still there, see fx_root_slot)
    const uint32_t maxprobe = A.status[kFxStMaxProbe];
    bool coll = false;
#pragma unroll
    for (int j = 0; j < kFxPts; ++j) coll = coll || (ok4[j] && found4[j] != key1[j] && (found4[j] != 0u || maxprobe != 0u));
    if (__ballot(coll)) {  // probe on (rare)
#pragma unroll
      for (int j = 0; j < kFxPts; ++j)
        if (ok4[j] && found4[j] != key1[j] && (found4[j] != 0u || maxprobe != 0u)) {
          const uint32_t r = fx_root_slot(A, key1[j], 0u, false, maxprobe);
          slot4[j] = r != 0xFFFFFFFFu ? r : 0u;
          found4[j] = r != 0xFFFFFFFFu ? key1[j] : 0u;
        }
    }
#pragma unroll
    for (int j = 0; j < kFxPts; ++j) {
      const bool present = ok4[j] && found4[j] == key1[j];
      const uint32_t *h32 = (const uint32_t *)(A.blk + (size_t)(present ? slot4[j] : 0u) * kFxBlockW);
      const uint2 sb = *(const uint2 *)(h32 + 12);
      split4[j] = present ? sb.x : 0u, base4[j] = present ? sb.y : 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < kFxPts; ++j) {
    const FxPt p = fx_pt_code<LEVEL>(A, base + j < n && fin[j], px[j], py[j], pz[j], pt[j], kxs[j], kys[j], kzs[j], k0x, k0y, k0z, split4[j], base4[j],
                                     bad_key, bad_time);
    code[j] = p.code, tmag[j] = p.tmag;
    qlx[j] = p.qlx, qly[j] = p.qly, qlz[j] = p.qlz;
  }
  }
  if (bad_key) raise_flag(A.status, kFlagKeyRange);
  if (bad_time) raise_flag(A.status, kFlagTimeRange);
  auto flush_lds = [&](unsigned long long code, const FxPart &a) -> bool {
    uint32_t s = fx_hash32((uint32_t)code ^ (uint32_t)(code >> 29)) & (kFxLds - 1);
    for (int probe = 0; probe < kFxLdsProbe; ++probe) {
      const unsigned long long old = atomicCAS(&h_key[s], 0ull, code);
      if (old == 0ull || old == code) {
        fx_add_cell(&h_rec[s][0], a);
        return true;
      }
      s = (s + 1) & (kFxLds - 1);
    }
    return false;  // the tile has more cells than its hash holds (within the probe limit): the caller spills the partial
  };

  // A partial sum is closed where the cell changes inside the lane (before point j = 1..3) and at the end of the lane (its
  // open partial, merged with the neighbouring lanes' below).  Few closings in a wavefront - a sweep with run structure -
  // become records in HBM right away (slot = rank among the wavefront's closings of that class: no atomics, no LDS); many
  // closings - no run structure - go through the tile's LDS hash, which merges the cells of the tile first.
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  bool bnd[kFxPts];
  unsigned long long ccode[kFxPts];  // class j < 3: the cell the lane closes in front of point j + 1; class 3: the lane's last cell
  {
    unsigned long long open = 0ull;
#pragma unroll
    for (int j = 0; j < kFxPts; ++j) {
      bnd[j] = code[j] != 0ull && open != 0ull && code[j] != open;
      if (j) ccode[j - 1] = open;
      if (code[j] != 0ull) open = code[j];
    }
    ccode[kFxPts - 1] = open;
  }
  // the run tails: the last lane of a run of equal last cells inside its row of 16 lanes (the segmented scan below sums the run into
  // it).  From the codes alone: the lane to the right in the row (row_shl:1; the row's last lane sees 0)
  bool tail;
  {
    const unsigned long long mycode = ccode[kFxPts - 1];
    const uint32_t nlo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)mycode, 0x101, 0xF, 0xF, true);
    const uint32_t nhi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(mycode >> 32), 0x101, 0xF, 0xF, true);
    const unsigned long long nextc = (unsigned long long)nlo | ((unsigned long long)nhi << 32);
    tail = mycode != 0ull && ((lane & 15) == 15 || nextc != mycode);
  }
  const uint32_t rec0 = bid * (uint32_t)kFxRecTile + (uint32_t)kFxLds + (uint32_t)wave * 4u * (uint32_t)kFxDirect;
  auto direct_ridx = [&](int cls, unsigned long long mclass) -> uint32_t {  // slot = rank among the wavefront's closings of the class
    return rec0 + (uint32_t)cls * (uint32_t)kFxDirect + (uint32_t)__popcll(mclass & lt_mask);
  };
  // THE route decision, in one place for the link and for the store: a class with at most kFxDirect closings in the wavefront
  // writes its records straight to HBM (mclass: the wavefront's closings of the class, not empty)
  auto direct_route = [](unsigned long long mclass) -> bool { return __popcll(mclass) <= kFxDirect; };
  // LINK EARLY (form bit 1): every class that takes the direct route is linked here, where its codes and record indices are known -
  // first the claims of all classes (one round trip for their hash probes), then the heads; the records follow from close_partial
  uint32_t l_old[kFxPts];
  bool l_ok[kFxPts];
#pragma unroll
  for (int cls = 0; cls < kFxPts; ++cls) l_old[cls] = 0u, l_ok[cls] = false;
  if (kLinkEarly && !(WC_DBG(P, 2))) {
    FxClaim claim[kFxPts];
#pragma unroll
    for (int cls = 0; cls < kFxPts; ++cls) {
      const bool closing = cls < 3 ? bnd[cls + 1] : tail;
      const unsigned long long mclass = __ballot(closing);
      if (mclass && direct_route(mclass)) claim[cls] = fx_link_claim<LEVEL>(A, closing, ccode[cls] & 0x7FFFFFFFFFFFFFFFull);
    }
#pragma unroll
    for (int cls = 0; cls < kFxPts; ++cls) {
      const bool closing = cls < 3 ? bnd[cls + 1] : tail;
      const unsigned long long mclass = __ballot(closing);
      if (mclass && direct_route(mclass))
        l_ok[cls] = fx_link_head<LEVEL>(A, closing, ccode[cls] & 0x7FFFFFFFFFFFFFFFull, sub, direct_ridx(cls, mclass), claim[cls], l_old[cls]);
    }
  }
  // WAVE-UNIFORM: `closing` marks the lanes that close a partial of class cls now
  auto close_partial = [&](int cls, bool closing, unsigned long long c, const FxPart &a) {
    const unsigned long long mclass = __ballot(closing);
    if (!mclass || (WC_DBG(P, 2))) return;
    if (direct_route(mclass)) {
      const uint32_t ridx = direct_ridx(cls, mclass);
      if (kLinkEarly) {
        if (closing && l_ok[cls]) fx_store<LEVEL>(A, c & 0x7FFFFFFFFFFFFFFFull, a, ridx, l_old[cls]);
      } else {
        fx_push<LEVEL>(A, closing, c & 0x7FFFFFFFFFFFFFFFull, a, sub, ridx);
      }
    } else {
      const bool failed = closing && !flush_lds(c, a);
      const unsigned long long mf = __ballot(failed);
      if (mf) {  // records from the spill pool: one atomic per wavefront on one of eight sub-counters
        const uint32_t sp = bid & 7u;
        uint32_t b0 = 0;
        if (lane == 0) b0 = atomicAdd(fx_cnt(A, kFxStSpillBank, sp), (uint32_t)__popcll(mf));
        b0 = (uint32_t)__shfl((int)b0, 0);
        const uint32_t k = b0 + (uint32_t)__popcll(mf & lt_mask);
        const bool room = k < A.spill_per;
        if (failed && !room) fx_fallback(A.status, 4);
        fx_push<LEVEL>(A, failed && room, c & 0x7FFFFFFFFFFFFFFFull, a, sub, A.rec_tiles * (uint32_t)kFxRecTile + sp * A.spill_per + k);
      }
    }
  };

  // ---- pass B: the partial sums, as RAW sums of magic-form bit patterns (see pass A); fx_fix turns them into the integers ----
  FxPart acc;
  double tlo_m = 0.0, thi_m = 0.0;  // smallest / largest tick of the open partial, magic form (0: none yet)
  uint32_t nfix = 0;                // points of the open partial whose share of n x bits(M) has been taken off already
  auto raw_zero = [&]() {
    fx_zero(acc);
    tlo_m = 1.0e300, thi_m = 0.0;
    nfix = 0;
  };
  // raw -> integer moments, IN PLACE (a second copy of the thirteen sums cost 25 registers and a wavefront per SIMD): what the points
  // added since the last call carry of n x bits(M) is taken off the high words; lanes that go on adding raw values afterwards are
  // corrected for those alone the next time (arithmetic mod 2^64)
  auto fx_fix = [&]() {
    const uint32_t dn = acc.n - nfix;
    nfix = acc.n;
    const unsigned long long c1 = (unsigned long long)(dn * kFxMagicHi) << 32, c2 = (unsigned long long)(dn * kFxMagic2Hi) << 32;
    acc.st = (long long)((unsigned long long)acc.st - c1);
#pragma unroll
    for (int i = 0; i < 3; ++i) acc.s[i] = (long long)((unsigned long long)acc.s[i] - c1);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc.ss[i] = (long long)((unsigned long long)acc.ss[i] - c2);
    const unsigned long long lo = (unsigned long long)__double_as_longlong(tlo_m) - kFxMagicBits, hi = (unsigned long long)__double_as_longlong(thi_m) - kFxMagicBits;
    acc.tmin_inv = acc.n ? kFxTMax - lo : 0ull;
    acc.tmax_p1 = acc.n ? hi + 1ull : 0ull;
  };
  raw_zero();
  unsigned long long cur = 0ull;
#pragma unroll
  for (int j = 0; j < kFxPts; ++j) {
    if (j) {
      if (__ballot(bnd[j])) {
        fx_fix();
        close_partial(j - 1, bnd[j], cur, acc);
      }
      if (bnd[j]) raw_zero();
    }
    if (code[j] == 0ull) continue;
    cur = code[j];
    acc.n += 1;
    acc.st += __double_as_longlong(tmag[j]);
    // the magic-form double again: high word = M's high word minus the borrow of a negative q
    const long long bx = (long long)(((unsigned long long)(kFxMagicHi - (qlx[j] >> 31)) << 32) | qlx[j]);
    const long long by = (long long)(((unsigned long long)(kFxMagicHi - (qly[j] >> 31)) << 32) | qly[j]);
    const long long bz = (long long)(((unsigned long long)(kFxMagicHi - (qlz[j] >> 31)) << 32) | qlz[j]);
    acc.s[0] += bx, acc.s[1] += by, acc.s[2] += bz;
    const double x = __longlong_as_double(bx) - kFxMagic, y = __longlong_as_double(by) - kFxMagic, z = __longlong_as_double(bz) - kFxMagic;
    acc.ss[0] += __double_as_longlong(fma(x, x, kFxMagic2)), acc.ss[1] += __double_as_longlong(fma(x, y, kFxMagic2));
    acc.ss[2] += __double_as_longlong(fma(x, z, kFxMagic2)), acc.ss[3] += __double_as_longlong(fma(y, y, kFxMagic2));
    acc.ss[4] += __double_as_longlong(fma(y, z, kFxMagic2)), acc.ss[5] += __double_as_longlong(fma(z, z, kFxMagic2));
    tlo_m = fmin(tlo_m, tmag[j]), thi_m = fmax(thi_m, tmag[j]);
  }
  fx_fix();  // the lane's open partial, as integers from here on
  // The lanes' open partials: neighbouring lanes hold consecutive points and mostly the same cell (a scan line stays in one
  // 0.4 m octant for tens of points), so runs of equal cells are summed across the lanes first - an inclusive segmented scan
  // INSIDE each row of 16 lanes, four steps of DPP row shifts (v_mov_b32_dpp row_shr: a full-rate VALU move; the same scan
  // over all 64 lanes with ds_bpermute shuffles took 5.9 k of the workgroup's 26 k clocks) - and only the LAST lane of a run
  // in its row closes the sum.  A run that crosses a row boundary leaves one record per row: records of a cell are added up by
  // k_fx_nodes anyway.
  {
    const unsigned long long mycode = acc.n ? cur : 0ull;
    auto shr32 = [](uint32_t v, auto dtag) -> uint32_t {  // value of the lane d to the left in the row, 0 at the row's start
      constexpr int d = decltype(dtag)::value;
      return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + d, 0xF, 0xF, true);
    };
    auto shr64 = [&](unsigned long long v, auto dtag) -> unsigned long long {
      return (unsigned long long)shr32((uint32_t)v, dtag) | ((unsigned long long)shr32((uint32_t)(v >> 32), dtag) << 32);
    };
    const int rl = lane & 15;
    const unsigned long long prevc = shr64(mycode, std::integral_constant<int, 1>{});
    uint32_t head = (rl == 0 || prevc != mycode) ? 1u : 0u;
    auto step = [&](auto dtag) {
      constexpr int d = decltype(dtag)::value;
      // (wave-uniform: a step moves 13 sums through ~75 instructions, and k_fx_acc is VALU-bound - 88 % busy at 10 M points by the SQ
      // counters, profiles/dev/sq_acc.sh.  No lane takes part in it when every run of the wavefront has found its head within d - 1
      // lanes: runs of at most 8 lanes - the patches of C2 - skip the last step, a sweep in firing order skips all four.)
      if (!__ballot(rl >= d && !head)) return;
      const uint32_t ohead = shr32(head, dtag);
      const uint32_t on = shr32(acc.n, dtag);
      const long long ost = (long long)shr64((unsigned long long)acc.st, dtag);
      long long os[3], oss[6];
#pragma unroll
      for (int i = 0; i < 3; ++i) os[i] = (long long)shr64((unsigned long long)acc.s[i], dtag);
#pragma unroll
      for (int i = 0; i < 6; ++i) oss[i] = (long long)shr64((unsigned long long)acc.ss[i], dtag);
      const unsigned long long omin = shr64(acc.tmin_inv, dtag), omax = shr64(acc.tmax_p1, dtag);
      if (rl >= d && !head) {
        acc.n += on, acc.st += ost;
#pragma unroll
        for (int i = 0; i < 3; ++i) acc.s[i] += os[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc.ss[i] += oss[i];
        acc.tmin_inv = max(acc.tmin_inv, omin);
        acc.tmax_p1 = max(acc.tmax_p1, omax);
        head = ohead;
      }
    };
    step(std::integral_constant<int, 1>{});
    step(std::integral_constant<int, 2>{});
    step(std::integral_constant<int, 4>{});
    step(std::integral_constant<int, 8>{});
    close_partial(3, tail, mycode, acc);
  }
  __syncthreads();
  // the tile's cells -> records in HBM
  if (WC_DBG(P, 1)) return;
  static_assert(kFxLds == kFxThreads, "one hash cell per thread in the final loop");
  {
    const int i = tid;
    const unsigned long long c = h_key[i];
    FxPart a;
    fx_zero(a);
    if (c != 0ull) {
      a.n = (uint32_t)h_rec[i][0];
      a.st = (long long)h_rec[i][1];
      for (int w = 0; w < 3; ++w) a.s[w] = (long long)h_rec[i][2 + w];
      for (int w = 0; w < 6; ++w) a.ss[w] = (long long)h_rec[i][5 + w];
      a.tmin_inv = h_rec[i][11];
      a.tmax_p1 = h_rec[i][12];
    }
    if (__ballot(c != 0ull)) fx_push<LEVEL>(A, c != 0ull, c & 0x7FFFFFFFFFFFFFFFull, a, sub, bid * (uint32_t)kFxRecTile + (uint32_t)i);
  }
}

// (Round 3 tried a PERSISTENT form - four workgroups per CU looping over the tiles, tile i + 1 requested before tile i is worked on,
// so that the loads would run behind the arithmetic: 156 VGPRs instead of 104, three wavefronts per SIMD, and SLOWER everywhere -
// 117 -> 172 us at 10 M points, 25 -> 28 us at 1 M.  One tile per workgroup stays.)
// (Round 5 tried it again for PACKED points, where the next tile is five 16-byte loads per lane held in 20 registers and needs no LDS
// staging: 168 VGPRs - three wavefronts per SIMD - and slower again with 2 / 3 / 4 workgroups per CU: 89 -> 134 / 114 / 124 us at 10 M
// points, 40 -> 57 / 47 / 53 at 4 M, 92 -> 129 / 105 / 132 on a 4 M-point room in firing order (profiles/dev/persist_acc.py ran them
// on one box).  Knock-out runs put the loads alone at 32 us, loads + arithmetic at 73, everything at 90: what adds up is not a load
// latency a prefetch could hide - with a quarter fewer wavefronts per CU the same instruction streams simply take longer.)
template <int LEVEL>
__global__ void __launch_bounds__(kFxThreads) k_fx_acc(FxArgs A) {
  fx_acc_body<LEVEL, kFxAccForm>(A, blockIdx.x);
}
// the other forms (development option fx_acc_form: tests and A/B runs), under a name of their own
template <int LEVEL, int FORM>
__global__ void __launch_bounds__(kFxThreads) k_fx_acc_form(FxArgs A) {
  fx_acc_body<LEVEL, FORM>(A, blockIdx.x);
}

// K sweeps in ONE launch (wc_extract_surfels_batch): workgroup -> (sweep k, tile) through the prefix table start[] (K + 1
// entries); each sweep has its own FxArgs - tables, records, control block - in B.args[k]
struct FxBatch {
  const FxArgs *args;      // [K]
  const uint32_t *start;   // [K + 1] first workgroup of every sweep in this launch
  const uint32_t *flags;   // [K] bit 0: the sweep takes part in the layer-2 launches, bit 1: in the list merge
  int K;
};
__device__ __forceinline__ int fx_batch_find(const FxBatch &B, uint32_t b, uint32_t &local) {
  int k = 0;
  while (k + 1 < B.K && b >= B.start[k + 1]) ++k;  // (K <= 64, uniform: scalar loads)
  local = b - B.start[k];
  return k;
}
// A sweep's arguments are copied into LDS first: read through the pointer, every field is a global load the compiler must repeat
// behind each store of the body (it cannot know that the argument array is not written: 267 vector loads in k_fx_acc_b against 56
// in k_fx_acc, 176 us against 134 for the same ten million points); LDS cannot alias the tables the body writes.
#define WC_FX_BATCH_ARGS(sA, B, k)                                                                 \
  __shared__ FxArgs sA;                                                                            \
  static_assert(sizeof(FxArgs) % 8 == 0, "copied as 64-bit words");                                 \
  for (uint32_t w_ = threadIdx.x; w_ < sizeof(FxArgs) / 8; w_ += blockDim.x)                      \
    ((unsigned long long *)&sA)[w_] = ((const unsigned long long *)&(B).args[k])[w_];              \
  __syncthreads();
template <int LEVEL>
__global__ void __launch_bounds__(kFxThreads) k_fx_acc_b(FxBatch B) {
  uint32_t bid;
  const int k = fx_batch_find(B, blockIdx.x, bid);
  if (LEVEL == 2 && !(B.flags[k] & 1u)) return;
  WC_FX_BATCH_ARGS(sA, B, k)
  fx_acc_body<LEVEL, kFxAccForm>(sA, bid);
}
template <int LEVEL, int FORM>
__global__ void __launch_bounds__(kFxThreads) k_fx_acc_form_b(FxBatch B) {
  uint32_t bid;
  const int k = fx_batch_find(B, blockIdx.x, bid);
  if (LEVEL == 2 && !(B.flags[k] & 1u)) return;
  WC_FX_BATCH_ARGS(sA, B, k)
  fx_acc_body<LEVEL, FORM>(sA, bid);
}
// host side: the kernel of the form the context asks for, or - option -1 - the library's choice: kFxAccForm (the default kernels)
// while one round of workgroups holds the sweep (up to 2 M points: the grid starts together and its phases would run one after the
// other - what both bits are for), bit 0 alone for a LARGER sweep on the staged path: there successive rounds of workgroups overlap
// already, and measured at 10 M points as records both bits together are slower than the kernel without either while bit 0 alone is
// faster (DESIGN 3.1); packed points keep kFxAccForm at every size (bit 1 gains 3 % at 10 M).  n = 0: a batch (kFxAccForm).
// Bit 0 does not apply to LEVEL 2: its forms are told apart by bit 1 alone, so that no instantiation exists twice under two names
constexpr uint64_t kFxAccResident = 2000000ull;  // (the bound of FxArgs::static_map: run_pipeline_fast)
inline int fx_acc_form_of(const wc_ctx *ctx, int level, uint64_t n, uint32_t fmt) {
  static_assert(kFxAccForm == 3, "fx_launch_acc / fx_launch_acc_b: the cases they name are the NON-default forms");
  int f = ctx->dev.fx_acc_form & 3;
  if (ctx->dev.fx_acc_form < 0) f = (n > kFxAccResident && fmt != 2u) ? 1 : kFxAccForm;
  return level == 2 ? ((f & 2) ? kFxAccForm : 0) : f;
}
template <int LEVEL>
void fx_launch_acc(const wc_ctx *ctx, unsigned grid, hipStream_t st, const FxArgs &A) {
  const int f = fx_acc_form_of(ctx, LEVEL, A.pts.n, A.fmt);
  if (f == 0) return (void)k_fx_acc_form<LEVEL, 0><<<grid, kFxThreads, 0, st>>>(A);
  if constexpr (LEVEL == 1) {
    if (f == 1) return (void)k_fx_acc_form<1, 1><<<grid, kFxThreads, 0, st>>>(A);
    if (f == 2) return (void)k_fx_acc_form<1, 2><<<grid, kFxThreads, 0, st>>>(A);
  }
  k_fx_acc<LEVEL><<<grid, kFxThreads, 0, st>>>(A);
}
template <int LEVEL>
void fx_launch_acc_b(const wc_ctx *ctx, unsigned grid, hipStream_t st, const FxBatch &B) {
  const int f = fx_acc_form_of(ctx, LEVEL, 0, 0u);
  if (f == 0) return (void)k_fx_acc_form_b<LEVEL, 0><<<grid, kFxThreads, 0, st>>>(B);
  if constexpr (LEVEL == 1) {
    if (f == 1) return (void)k_fx_acc_form_b<1, 1><<<grid, kFxThreads, 0, st>>>(B);
    if (f == 2) return (void)k_fx_acc_form_b<1, 2><<<grid, kFxThreads, 0, st>>>(B);
  }
  k_fx_acc_b<LEVEL><<<grid, kFxThreads, 0, st>>>(B);
}

// ---- long lists: one record per (node, time slot) --------------------------------------------------------------------------
// A sweep without run structure leaves several records per cell (one per tile that touched it: 2.3 on average in a 1 M-point
// sweep in firing order, 12 in the busiest time bin, 59 in the busiest node), and k_fx_nodes - one lane per node - walks a node's
// lists record by record: the busiest node of the sweep set the duration of the whole kernel (28 of 46 us of its slowest
// wavefront in the walk).  This kernel gives every LIST its own lane first: the lane adds the list's records up and writes the
// sum back into the list's first record (next = 0); the nodes kernel then finds lists of one record.  Launched when the previous
// sweep reported long walks (k_fx_nodes raises mailbox word 15); a list whose records do not share one time bin is left alone
// (k_fx_nodes flags it).  One workgroup of 128 lanes per parent (8 children x 16 time slots).
template <int LEVEL>
__device__ __forceinline__ void fx_merge_body(const FxArgs &A, const uint32_t bid, const uint32_t nblk) {
  const uint32_t bank = LEVEL == 1 ? kFxStRoots : kFxStNodes2;
  const uint32_t per = LEVEL == 1 ? A.mr_per : A.mq_per;
  uint32_t total = 0, cnts[kFxSub];
#pragma unroll
  for (int j = 0; j < kFxSub; ++j) {
    cnts[j] = min(*fx_cnt(A, bank, j), per);
    total += cnts[j];
  }
  for (uint32_t gi = bid; gi < total; gi += nblk) {
    uint32_t pidx = 0, rem = gi;
    bool found = false;
#pragma unroll
    for (int j = 0; j < kFxSub; ++j) {
      if (!found) {
        if (rem < cnts[j]) {
          pidx = (uint32_t)j * per + rem;
          found = true;
        } else {
          rem -= cnts[j];
        }
      }
    }
    if (LEVEL == 1) pidx = A.rlist[pidx];
    const unsigned long long *blk = (LEVEL == 1 ? A.blk : A.blk2) + (size_t)pidx * kFxBlockW;
    const uint32_t head = ((const uint32_t *)(blk + kFxHdrW))[threadIdx.x];
    if (head == 0u) continue;
    unsigned long long *first = A.rec + ((size_t)(LEVEL - 1) * A.rec_cap + (head - 1u)) * kFxRecW;
    ulonglong2 *f2 = (ulonglong2 *)first;
    const ulonglong2 w0 = f2[0], w6 = f2[6];
    uint32_t idx = (uint32_t)w6.y;
    if (idx == 0u) continue;  // one record: nothing to do
    const ulonglong2 w1 = f2[1], w2 = f2[2], w3 = f2[3], w4 = f2[4], w5 = f2[5];
    const uint32_t bin = (uint32_t)(w0.x >> 32);
    FxPart b;
    b.n = (uint32_t)w0.x, b.st = (long long)w0.y;
    b.s[0] = (long long)w1.x, b.s[1] = (long long)w1.y, b.s[2] = (long long)w2.x;
    b.ss[0] = (long long)w2.y, b.ss[1] = (long long)w3.x, b.ss[2] = (long long)w3.y;
    b.ss[3] = (long long)w4.x, b.ss[4] = (long long)w4.y, b.ss[5] = (long long)w5.x;
    b.tmin_inv = w5.y, b.tmax_p1 = w6.x;
    bool same = true;
    int guard = 0;
    for (; idx != 0u && guard < 100000; ++guard) {
      const ulonglong2 *r2 = (const ulonglong2 *)(A.rec + ((size_t)(LEVEL - 1) * A.rec_cap + (idx - 1u)) * kFxRecW);
      const ulonglong2 v0 = r2[0], v1 = r2[1], v2 = r2[2], v3 = r2[3], v4 = r2[4], v5 = r2[5], v6 = r2[6];
      same = same && (uint32_t)(v0.x >> 32) == bin;
      b.n += (uint32_t)v0.x, b.st += (long long)v0.y;
      b.s[0] += (long long)v1.x, b.s[1] += (long long)v1.y, b.s[2] += (long long)v2.x;
      b.ss[0] += (long long)v2.y, b.ss[1] += (long long)v3.x, b.ss[2] += (long long)v3.y;
      b.ss[3] += (long long)v4.x, b.ss[4] += (long long)v4.y, b.ss[5] += (long long)v5.x;
      b.tmin_inv = max(b.tmin_inv, v5.y), b.tmax_p1 = max(b.tmax_p1, v6.x);
      idx = (uint32_t)v6.y;
    }
    if (guard >= A.P.merge_min) {  // (keeps this kernel in the next sweep's launch sequence: k_fx_nodes will not see the long list any more)
      uint32_t *hm = host_mailbox(A.status);
      if (hm) hm[LEVEL == 1 ? 15 : 16] = 1u;  // (a word per level: the next sweep merges only the level that had long lists)
    }
    if (!same || idx != 0u) continue;
    f2[0] = make_ulonglong2((unsigned long long)b.n | ((unsigned long long)bin << 32), (unsigned long long)b.st);
    f2[1] = make_ulonglong2((unsigned long long)b.s[0], (unsigned long long)b.s[1]);
    f2[2] = make_ulonglong2((unsigned long long)b.s[2], (unsigned long long)b.ss[0]);
    f2[3] = make_ulonglong2((unsigned long long)b.ss[1], (unsigned long long)b.ss[2]);
    f2[4] = make_ulonglong2((unsigned long long)b.ss[3], (unsigned long long)b.ss[4]);
    f2[5] = make_ulonglong2((unsigned long long)b.ss[5], b.tmin_inv);
    f2[6] = make_ulonglong2(b.tmax_p1, 0ull);
  }
}

template <int LEVEL>
__global__ void __launch_bounds__(128) k_fx_merge(FxArgs A) {
  fx_merge_body<LEVEL>(A, blockIdx.x, gridDim.x);
}
template <int LEVEL>
__global__ void __launch_bounds__(128) k_fx_merge_b(FxBatch B) {
  uint32_t bid;
  const int k = fx_batch_find(B, blockIdx.x, bid);
  if (!(B.flags[k] & 2u) || (LEVEL == 2 && !(B.flags[k] & 1u))) return;
  WC_FX_BATCH_ARGS(sA, B, k)
  fx_merge_body<LEVEL>(sA, bid, B.start[k + 1] - B.start[k]);
}

// ---- node tests, temporal clusters, emission --------------------------------------------------------------------------------
__device__ __forceinline__ long long fx_gsum8(long long v) {  // sum over the 8 lanes of a group, result in every lane
  for (int m = 1; m < 8; m <<= 1) v += __shfl_xor(v, m, 8);
  return v;
}
__device__ __forceinline__ void fx_gsum8(FxPart &a) {
  a.n = (uint32_t)fx_gsum8((long long)a.n);
  a.st = fx_gsum8(a.st);
  for (int i = 0; i < 3; ++i) a.s[i] = fx_gsum8(a.s[i]);
  for (int i = 0; i < 6; ++i) a.ss[i] = fx_gsum8(a.ss[i]);
}

#include "fx_eig3.h"

struct FxPca {
  Pca r;
  bool near;  // a gate closer to its threshold than the reference's own rounding noise
  int which;  // ... which one: 0 the eigenvalue threshold, 1 the likeness, 2 a non-positive trace (wc_debug_status words 49 ... 51)
};

// integer moments (relative to the rounded voxel centre cc) -> mean, covariance, eigen-decomposition, gate margins
__device__ __forceinline__ void fx_pca(const FxArgs &A, const FxPart &m, const double *cc, FxPca &o) {
  const double n = (double)m.n;
  // (one division: the moments are exact integers, the quotients are rounded once either way; ten dependent fp64 divisions
  // were a fifth of this routine, and the routine is 40 % of a k_fx_nodes wavefront)
  const double in = fx_rcp(n), iq = A.inv_q * in, iqq = A.inv_qq * in;
  const double mx = (double)m.s[0] * iq, my = (double)m.s[1] * iq, mz = (double)m.s[2] * iq;
  wc::M3 C;
  C.m[0][0] = (double)m.ss[0] * iqq - mx * mx;
  C.m[0][1] = C.m[1][0] = (double)m.ss[1] * iqq - mx * my;
  C.m[0][2] = C.m[2][0] = (double)m.ss[2] * iqq - mx * mz;
  C.m[1][1] = (double)m.ss[3] * iqq - my * my;
  C.m[1][2] = C.m[2][1] = (double)m.ss[4] * iqq - my * mz;
  C.m[2][2] = (double)m.ss[5] * iqq - mz * mz;
  Pca &r = o.r;
  r.c[0] = cc[0] + mx, r.c[1] = cc[1] + my, r.c[2] = cc[2] + mz;
  r.tmean = A.t_lo + ((double)m.st * in) * A.inv_tick;
  wc::M3 V;
  fx_eig3(C, r.ev, V);
  for (int i = 0; i < 3; ++i) {
    r.nrm[i] = V.m[i][0];
    for (int j = 0; j < 3; ++j) r.cov[3 * i + j] = C.m[i][j];
  }
  const double sum = (r.ev[0] + r.ev[1]) + r.ev[2];
  const double isum = fx_rcp(sum);
  r.like = 2 * (r.ev[1] - r.ev[0]) * isum;
  // The reference forms sum(p p^T)/n - c c^T in fp64 on world coordinates (cc:40-47, :89-97): rounding noise of the order
  // sqrt(n) |c|^2 eps in every covariance entry (SURVEY Q6).  A gate inside that band (x16) is not decided here - nor one inside
  // THIS path's own error: its covariance entries are off by up to B_cov = 2^-45 (the product grid) + 2 2^-33 vs f (coordinates below
  // 2^-8 m are finer than the 2^-32 m grid; f: the share of such points) + 16 2^-53 (vs/2)^2, lambda_0 by up to 3 B_cov (DESIGN 4.3).
  // A.band0 = 1e-14 + 3 B_cov with f = 1, a constant of the sweep.  (Without it a root with its lower half in 0 < x < 2^-9 m, lambda_0
  // 5e-12 above the threshold - 42 of the narrower bands - came out a plane: tests/test_extract_gates_gpu.py, lam0-root-slab.)
  const double R2 = r.c[0] * r.c[0] + r.c[1] * r.c[1] + r.c[2] * r.c[2] + 1.0;
  const double dl = 16.0 * (n * fx_rsqrt(n)) * R2 * 1.1102230246251565e-16 + A.band0;
  const double dlike = 6.0 * dl * fabs(isum) + 1e-13;
  // (Round 5 also sent a smallest eigenvalue inside that band of ZERO to the exact path - the reference's sigma = sqrt(lambda_0) is then NaN
  // or a rounding-sized number by the luck of its own sums - and took it out again: such clusters are not rare, every stretch of ONE scan
  // line on a surface is one (its points span a plane exactly: line direction x ray direction), and from ~2 M points per sweep on every
  // room sweep carried one and was repeated on the exact path.  The default arithmetic returns the sigma its exact sums give; where the
  // reference's own value is noise the tests compare nothing: tests/helpers.py.)
  o.near = (fabs(r.ev[0] - A.P.thr) <= dl) || (fabs(r.like - A.P.min_like) <= dlike) || !(sum > 0.0);
  o.which = (fabs(r.ev[0] - A.P.thr) <= dl) ? 0 : ((fabs(r.like - A.P.min_like) <= dlike) ? 1 : 2);
}

// A node whose smallest eigenvalue PROVABLY lies above the plane threshold needs no eigen-decomposition: it is not a plane whatever its
// likeness (cc:106-111 is a conjunction), nothing is emitted for it, and its eigenvector is never used.  For a symmetric positive
// semi-definite C: lambda_0 = det C / (lambda_1 lambda_2) >= det C / ((lambda_1 + lambda_2) / 2)^2 >= 4 det C / tr(C)^2.  The bound is
// compared with the threshold plus the band fx_pca calls "near" (and 0.1 % on top for the rounding of det and tr): where it holds the
// gate is not near its threshold either.  What it buys: the ROOT of a voxel that holds several surfaces - every root of a scene made
// of patches, C2 - is tested by eight lanes of a wavefront while 56 wait, a chain of ~5 k clocks of k_fx_nodes' ~26 k.
__device__ __forceinline__ bool fx_surely_not_plane(const FxArgs &A, const FxPart &m, const double *cc) {
  const double n = (double)m.n;
  const double in = fx_rcp(n), iq = A.inv_q * in, iqq = A.inv_qq * in;
  const double mx = (double)m.s[0] * iq, my = (double)m.s[1] * iq, mz = (double)m.s[2] * iq;
  const double c00 = (double)m.ss[0] * iqq - mx * mx, c01 = (double)m.ss[1] * iqq - mx * my, c02 = (double)m.ss[2] * iqq - mx * mz;
  const double c11 = (double)m.ss[3] * iqq - my * my, c12 = (double)m.ss[4] * iqq - my * mz, c22 = (double)m.ss[5] * iqq - mz * mz;
  const double det = c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) + c02 * (c01 * c12 - c11 * c02);
  const double tr = (c00 + c11) + c22;
  const double px = cc[0] + mx, py = cc[1] + my, pz = cc[2] + mz;
  const double R2 = px * px + py * py + pz * pz + 1.0;
  const double dl = 16.0 * (n * fx_rsqrt(n)) * R2 * 1.1102230246251565e-16 + A.band0;  // (fx_pca's band)
  return m.n != 0u && tr > 0.0 && 4.0 * det > 1.001 * (A.P.thr + dl) * tr * tr;
}

// the emission of a surfel in two parts: fx_emit_begin stores it and asks for its place in its time bucket (an atomic WITH
// return: a round trip), fx_emit_end stores the (key, slot) entry there - whatever is put between the two runs while the
// atomic is under way
struct FxEmit {
  uint64_t entry;
  uint32_t bkt, r, rank;  // r: what the bucket counter returned, in the lane `lead` that asked for the whole group
  int lead;
  bool on;
};
// (every lane that emits must arrive here together with the leader of its group: the callers do not separate them)
__device__ __forceinline__ void fx_emit_end(const FxArgs &A, const FxEmit &e) {
  const uint32_t r = (uint32_t)__shfl((int)e.r, e.lead) + e.rank;
  if (e.on && r < A.slot_bin_cap) A.slot_bins[(size_t)e.bkt * A.slot_bin_cap + r] = e.entry;
}
__device__ __forceinline__ FxEmit fx_emit_begin(const FxArgs &A, const Pca &rr, uint32_t slot, int layer, uint32_t o1, uint32_t o2, uint32_t ord, int kx,
                                                int ky, int kz, float q0) {
  const ExParams &P = A.P;
  double nx = rr.nrm[0], ny = rr.nrm[1], nz = rr.nrm[2];
  const double d = nx * (rr.c[0] - P.view[0]) + ny * (rr.c[1] - P.view[1]) + nz * (rr.c[2] - P.view[2]);
  if (d < 0) nx = -nx, ny = -ny, nz = -nz;  // cc:59-61
  const float ql = layer == 0 ? q0 : (layer == 1 ? q0 / 2 : (q0 / 2) / 2);
  wc_surfel sf;
  sf.t = rr.tmean;
  sf.center[0] = rr.c[0], sf.center[1] = rr.c[1], sf.center[2] = rr.c[2];
  for (int i = 0; i < 9; ++i) sf.cov[i] = rr.cov[i];
  sf.normal[0] = nx, sf.normal[1] = ny, sf.normal[2] = nz;
  sf.resolution = (double)(ql * 4);  // quarter_length_ * 4, float arithmetic (cc:307)
  sf.sigma = sqrt(rr.ev[0]);
  A.slots[slot] = sf;
  uint32_t node = (uint32_t)layer;
  if (layer >= 1) node |= o1 << 2;
  if (layer == 2) node |= o2 << 5;
  A.slot_ids[slot] = wc_surfel_id{kx, ky, kz, node | (ord << 8)};
  // time key of the surfel order: the stamp as a 32-bit fraction of [t_lo, t_hi] (monotone; k_slot_emit compares the stamps
  // themselves where keys collide), whatever the magnitude of the stamps
  const double frac = (rr.tmean - A.t_lo) * A.inv_span;
  if (!(frac >= 0.0 && frac <= 1.0)) raise_flag(A.status, kFlagTimeRange);
  const uint64_t key = (uint64_t)min(max(frac, 0.0) * 4294967296.0, 4294967295.0);
  FxEmit e;
  e.on = true;
  e.bkt = (uint32_t)(key >> 20);
  e.entry = (key << 32) | (uint64_t)slot;
  // place in the time bucket: ONE atomic per distinct bucket of the wavefront's emitting lanes (the surfels a wavefront emits in
  // one go are neighbours in time - one or two buckets - and 64 atomics on one word, or on the 32 counters sharing its 128-byte
  // line, are served one after the other: 312 k of them were most of this stage at 10 M points).  The leaders of all distinct
  // buckets issue their atomics in ONE instruction; nobody waits for the answer here (fx_emit_end hands it to the group).
  // Called under divergence: the ballots see the emitting lanes only.
  const int lane = threadIdx.x & 63;
  e.lead = lane, e.rank = 0;
  uint32_t gsize = 1;
  if (!(WC_DBG(P, 16384))) {  // (profiling knob: one atomic per surfel, as in round 2)
    unsigned long long todo = __ballot(true);
    // (at most four groups: lanes that are still alone after that - a sweep in firing order, whose surfels are spread over the
    // whole time range - ask for themselves)
    for (int round = 0; todo && round < 4; ++round) {
      const int lead = __ffsll((long long)todo) - 1;
      const uint32_t b0 = (uint32_t)__shfl((int)e.bkt, lead);
      const bool mine = e.bkt == b0;
      const unsigned long long m = __ballot(mine);
      if (mine) e.lead = lead, e.rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), gsize = (uint32_t)__popcll(m);
      todo &= ~m;
    }
  }
  e.r = 0;
  if (e.lead == lane) e.r = atomicAdd(&A.slot_counts[e.bkt], gsize);
  return e;
}
__device__ __forceinline__ void fx_emit(const FxArgs &A, const Pca &rr, uint32_t slot, int layer, uint32_t o1, uint32_t o2, uint32_t ord, int kx,
                                        int ky, int kz, float q0) {
  fx_emit_end(A, fx_emit_begin(A, rr, slot, layer, o1, o2, ord, kx, ky, kz, q0));
}

// kFxChains lists at a time: the next record of each (the loads of all four in flight together; a finished list re-reads record
// 0 and adds nothing - no branch for the compiler to hide a load behind).  bin[j] = the time bin list j must hold.
constexpr int kFxChains = 4;
constexpr int kFxJobCap = 512;  // jobs per wavefront of k_fx_nodes (64 children + 8 roots, clusters with >= cluster_min points)
constexpr int kFxJobW = 12;     // u64 words per job: n | ord << 32, St, Sq[3], Sqq[6], spare
template <int N, int CAP = kFxChains>
__device__ __forceinline__ void fx_stepn(const FxArgs &A, int level, uint32_t (&ix)[CAP], const uint32_t (&bin)[CAP], FxPart (&b)[CAP]) {
  const unsigned long long *base = A.rec + (size_t)(level - 1) * A.rec_cap * kFxRecW;
  ulonglong2 w[N][7];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const ulonglong2 *r2 = (const ulonglong2 *)(base + (size_t)(ix[j] ? ix[j] - 1u : 0u) * kFxRecW);
#pragma unroll
    for (int i = 0; i < 7; ++i) w[j][i] = r2[i];
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool on = ix[j] != 0u;
    const unsigned long long m = on ? ~0ull : 0ull;
    if (on && (uint32_t)(w[j][0].x >> 32) != bin[j]) fx_fallback(A.status, 6);  // two bins of this node 16 apart share the slot: > 0.75 s in one node
    FxPart &q = b[j];
    q.n += (uint32_t)(w[j][0].x & m);
    q.st += (long long)(w[j][0].y & m);
    q.s[0] += (long long)(w[j][1].x & m), q.s[1] += (long long)(w[j][1].y & m), q.s[2] += (long long)(w[j][2].x & m);
    q.ss[0] += (long long)(w[j][2].y & m), q.ss[1] += (long long)(w[j][3].x & m), q.ss[2] += (long long)(w[j][3].y & m);
    q.ss[3] += (long long)(w[j][4].x & m), q.ss[4] += (long long)(w[j][4].y & m), q.ss[5] += (long long)(w[j][5].x & m);
    q.tmin_inv = max(q.tmin_inv, w[j][5].y & m);
    q.tmax_p1 = max(q.tmax_p1, w[j][6].x & m);
    ix[j] = (uint32_t)(w[j][6].y & m);
  }
}
// ---- the node stage's routines.  Both of its forms are built from them: k_fx_nodes below (one launch) and k_fx_walk + k_fx_test
//      (extract_split.inc, two launches).  A "parent" is a root voxel (LEVEL 1: its node is layer 0, its children the layer-1
//      octants) or a queued layer-1 node (LEVEL 2: already tested and found not to be a plane, cc:175-182; children = its layer-2
//      octants).  8 lanes per parent, lane = child octant; eight parents per wavefront ----

// the fx_fallback codes of a form's call sites (wc_debug_status reports which of them fired)
struct FxWhy {
  int gap;        // a gap between time bins too near the cluster gap to be decided on ticks
  int slots;      // the wavefront's slot sub-range is full
  int jobs;       // the wavefront's job staging area is full
  int walk1;      // a list walk that does not end (one chain / several chains)
  int walkn;
  int big_bin;    // a time bin with more than 2^20 points
  int job_which;  // first of the three codes naming the gate a job's PCA was near (FxPca::which); < 0: not reported
};

// the parents sit in kFxSub dense sub-lists (one counter each), handed out back to back: entry gi of them all -> block index
template <int LEVEL>
__device__ __forceinline__ uint32_t fx_dense_parent(const FxArgs &A, const uint32_t (&cnts)[kFxSub], uint32_t per, uint32_t gi, bool have_parent) {
  uint32_t pidx = 0;
  if (have_parent) {
    uint32_t rem = gi;
    bool found = false;
#pragma unroll
    for (int j = 0; j < kFxSub; ++j) {
      const uint32_t cj = cnts[j];
      if (!found) {
        if (rem < cj) {
          pidx = (uint32_t)j * per + rem;
          found = true;
        } else {
          rem -= cj;
        }
      }
    }
  }
  if (LEVEL == 1 && have_parent) pidx = A.rlist[pidx];  // dense list entry -> hash slot = block index
  return pidx;
}

// the parent's header: its first time bin, its root key and (LEVEL 2) its layer-1 octant
template <int LEVEL>
__device__ __forceinline__ void fx_parent_header(const FxArgs &A, const unsigned long long *blk, uint32_t pidx, bool have_parent, uint32_t &key,
                                                 uint32_t &o1p, uint32_t &minbin) {
  const uint32_t *h32 = (const uint32_t *)blk;
  key = 0, o1p = 0, minbin = 0;
  if (have_parent) {
    minbin = 0xFFFFFFFFu - h32[2];
    if (LEVEL == 1) {
      key = A.rkey[pidx] - 1u;
    } else {  // header of a queued node (written when it was queued): word 0 = root slot | o1 << 28 | first-child flag << 31,
      const uint32_t ro = h32[0];  // word 1 = root key + 1
      o1p = (ro >> 28) & 7u;
      key = h32[1] - 1u;
    }
  }
}

// root key -> voxel index (k0: the voxel of the sweep's first point) and the voxel centre itself (k_fx_acc's reference point)
__device__ __forceinline__ void fx_key_voxel(const ExParams &P, uint32_t key, int k0x, int k0y, int k0z, int &kx, int &ky, int &kz, double (&cc)[3]) {
  kx = (int)(key & 1023u) - 512 + k0x, ky = (int)((key >> 10) & 1023u) - 512 + k0y, kz = (int)(key >> 20) - 512 + k0z;
  cc[0] = (0.5 + kx) * P.vs_f, cc[1] = (0.5 + ky) * P.vs_f, cc[2] = (0.5 + kz) * P.vs_f;
}

// the 16 list heads of this lane's child, in time order: position p holds bin minbin + p.  They live in LDS (the walks index them
// dynamically; a register array would go to scratch memory).  Returns the positions with a list
__device__ __forceinline__ uint32_t fx_load_heads(const unsigned long long *blk, bool have_parent, uint32_t minbin, uint32_t *heads) {
  uint32_t occ = 0;
  // (the loads do not wait for minbin: slot s goes to position (s - minbin) mod 16)
  const uint4 *hq = (const uint4 *)(blk + kFxHdrW) + (threadIdx.x & 7) * (kFxSlots / 4);
  uint32_t hv[kFxSlots];
#pragma unroll
  for (int q = 0; q < kFxSlots / 4; ++q) {
    const uint4 v = have_parent ? hq[q] : make_uint4(0u, 0u, 0u, 0u);
    hv[4 * q] = v.x, hv[4 * q + 1] = v.y, hv[4 * q + 2] = v.z, hv[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int s = 0; s < kFxSlots; ++s) {
    const uint32_t p = ((uint32_t)s - minbin) & (kFxSlots - 1);
    heads[p] = hv[s];
    if (hv[s]) occ |= 1u << p;
  }
  __builtin_amdgcn_wave_barrier();
  return occ;
}

__device__ __forceinline__ double fx_tick_time(const FxArgs &A, unsigned long long tk) { return A.t_lo + (double)tk * A.inv_tick; }  // exact inverse of k_fx_acc's tick
// does a new temporal cluster start at a bin whose first tick is tmin, after a bin whose last tick + 1 is prev_p1 (cc:24)?
__device__ __forceinline__ bool fx_starts(const FxArgs &A, unsigned long long tmin, unsigned long long prev_p1, int why) {
  if (prev_p1 == 0ull) return true;
  const double dt = fx_tick_time(A, tmin) - fx_tick_time(A, prev_p1 - 1ull);
  if (fabs(dt - A.P.gap) <= 8.0 * A.inv_tick) fx_fallback(A.status, why);  // ticks may be rounded: do not decide here
  return dt > A.P.gap;
}

// slots: every wavefront takes what it needs from its sub-range wsub with one atomic per round; the atomic can be issued ahead of
// the work that decides who really needs a slot (a slot taken in vain is a hole nobody refers to)
__device__ __forceinline__ uint32_t fx_slots_issue(const FxArgs &A, uint32_t wsub, bool want, unsigned long long &m) {
  m = __ballot(want);
  uint32_t base_ = 0;
  if (m && threadIdx.x == 0) base_ = atomicAdd(fx_cnt(A, kFxStSlots, wsub), (uint32_t)__popcll(m));
  return base_;
}
__device__ __forceinline__ uint32_t fx_slots_finish(const FxArgs &A, uint32_t wsub, bool want, unsigned long long m, uint32_t base_, int why) {
  if (!m) return 0xFFFFFFFFu;
  base_ = (uint32_t)__shfl((int)base_, 0);
  const uint32_t local = base_ + (uint32_t)__popcll(m & ((1ull << threadIdx.x) - 1ull));
  if (want && local >= A.slots_per) {
    fx_fallback(A.status, why);
    return 0xFFFFFFFFu;
  }
  return wsub * A.slots_per + local;
}
__device__ __forceinline__ uint32_t fx_take_slots(const FxArgs &A, uint32_t wsub, bool want, int why) {
  unsigned long long m;
  const uint32_t b = fx_slots_issue(A, wsub, want, m);
  return fx_slots_finish(A, wsub, want, m, b, why);
}

// a closing cluster with cluster_min points or more is put aside as a job (word 11: its owner, the lane of the child or 64 + group
// for a root) in the wavefront's staging area jb.  WAVE-UNIFORM call.  Returns the job's position in the lane that stored one,
// kFxJobCap in every other lane
__device__ __forceinline__ uint32_t fx_push_job(const FxArgs &A, unsigned long long *jb, uint32_t &jcnt, bool closing, const FxPart &cl, uint32_t ordv,
                                                uint32_t owner, int why) {
  const bool want = closing && (int)cl.n >= A.P.cluster_min;
  const unsigned long long m = __ballot(want);
  if (!m) return (uint32_t)kFxJobCap;
  const uint32_t pos = jcnt + (uint32_t)__popcll(m & ((1ull << threadIdx.x) - 1ull));
  jcnt += (uint32_t)__popcll(m);
  if (!want) return (uint32_t)kFxJobCap;
  if (pos >= (uint32_t)kFxJobCap) {
    fx_fallback(A.status, why);
    return (uint32_t)kFxJobCap;
  }
  ulonglong2 *o = (ulonglong2 *)(jb + (size_t)pos * kFxJobW);
  o[0] = make_ulonglong2((unsigned long long)cl.n | ((unsigned long long)ordv << 32), (unsigned long long)cl.st);
  o[1] = make_ulonglong2((unsigned long long)cl.s[0], (unsigned long long)cl.s[1]);
  o[2] = make_ulonglong2((unsigned long long)cl.s[2], (unsigned long long)cl.ss[0]);
  o[3] = make_ulonglong2((unsigned long long)cl.ss[1], (unsigned long long)cl.ss[2]);
  o[4] = make_ulonglong2((unsigned long long)cl.ss[3], (unsigned long long)cl.ss[4]);
  o[5] = make_ulonglong2((unsigned long long)cl.ss[5], (unsigned long long)owner);
  return pos;
}

// Every lane walks the record lists of its node CHAINS TIME BINS AT A TIME (independent lists: that many records in flight per lane -
// a single list is one dependent HBM round trip per record, and the busiest node of the sweep sets the kernel's duration), then
// handles the finished bins in time order: node total, temporal clusters (ClusterSurfels' first loop, cc:19-29).  Whether the node is
// a plane is only known at the end, so every cluster that closes with enough points is put aside as a JOB (push_job); the jobs of the
// nodes that turn out to be planes with several clusters get their PCA afterwards, 64 at a time - one lane per job, whoever owns it.
// add_root: every bin is also added to the parent's root node (root: its 16 time bins in LDS; ds atomics, the eight children of a
// root share the bin).
template <int LEVEL, int CHAINS, class PushJob>
__device__ __forceinline__ void fx_walk_node(const FxArgs &A, uint32_t occ, uint32_t minbin, const uint32_t *heads, bool add_root,
                                             unsigned long long (*root)[13], const FxWhy &why, PushJob &push_job, FxPart &tot, uint32_t &ncl) {
  fx_zero(tot);
  ncl = 0;
  uint32_t todo = (WC_DBG(A.P, 512)) ? 0u : occ;
  unsigned long long prev_p1 = 0ull;
  FxPart cur;
  fx_zero(cur);
  uint32_t ord = 0;
  while (__ballot(todo != 0u)) {
    uint32_t ix[CHAINS], bn[CHAINS];
    int pj[CHAINS];
    FxPart b[CHAINS];
#pragma unroll
    for (int j = 0; j < CHAINS; ++j) {
      fx_zero(b[j]);
      pj[j] = 0, ix[j] = 0u;
      if (todo) {
        pj[j] = __ffs((int)todo) - 1;
        todo &= todo - 1u;
        ix[j] = heads[pj[j]];
      }
      bn[j] = minbin + (uint32_t)pj[j];
    }
    int guard = 0;
    const bool several = __ballot(ix[1] != 0u) != 0ull;  // (a sweep with run structure: one bin per node, one list)
    if (!several) {
      while (__ballot(ix[0] != 0u)) {
        fx_stepn<1, CHAINS>(A, LEVEL, ix, bn, b);
        if (++guard > 200000) {
          fx_fallback(A.status, why.walk1);
          break;
        }
      }
    } else {
      for (;;) {
        uint32_t any = 0u;
#pragma unroll
        for (int j = 0; j < CHAINS; ++j) any |= ix[j];
        if (!__ballot(any != 0u)) break;
        fx_stepn<CHAINS, CHAINS>(A, LEVEL, ix, bn, b);
        if (++guard > 200000) {
          fx_fallback(A.status, why.walkn);
          break;
        }
      }
      if (guard > A.P.merge_min && threadIdx.x == 0) {  // lists of more than three records: the next sweep merges them first (k_fx_merge)
        uint32_t *hm = host_mailbox(A.status);
        if (hm) hm[LEVEL == 1 ? 15 : 16] = 1u;  // (a word per level: the next sweep merges only the level that had long lists)
      }
    }
#pragma unroll
    for (int j = 0; j < CHAINS; ++j) {
      if (j > 0 && !several) break;
      const bool have = b[j].n != 0u;
      bool closing = false;
      if (have) {
        if (b[j].n > (1u << 20)) fx_fallback(A.status, why.big_bin);  // 2^42 x n must stay below 2^63
        if (fx_starts(A, kFxTMax - b[j].tmin_inv, prev_p1, why.gap)) {
          ++ncl;
          closing = cur.n != 0u;
        }
        prev_p1 = b[j].tmax_p1;
        fx_acc(tot, b[j]);
        if (add_root) fx_add_cell(&root[pj[j]][0], b[j]);
      }
      push_job(closing, cur, ord, (uint32_t)threadIdx.x);
      if (closing) {
        ++ord;
        fx_zero(cur);
      }
      if (have) fx_acc(cur, b[j]);
    }
  }
  push_job(ncl > 1u, cur, ord, (uint32_t)threadIdx.x);  // the last of several clusters (a single one is the node itself)
}

// the temporal clusters of the root node of this lane's group (lanes with `on`) from its time bins, summed over the children in
// LDS (root); closed clusters go to push_job.  Returns their number
template <class PushJob>
__device__ __forceinline__ uint32_t fx_root_clusters(const FxArgs &A, bool on, const unsigned long long (*root)[13], int why_gap, PushJob &push_job) {
  const uint32_t owner = 64u + (uint32_t)(threadIdx.x >> 3);
  uint32_t root_ncl = 0;
  FxPart cur;
  fx_zero(cur);
  unsigned long long prev_p1 = 0ull;
  uint32_t ord = 0;
  for (int p = 0; p < kFxSlots; ++p) {
    bool closing = false;
    FxPart b;
    fx_zero(b);
    if (on) {
      const unsigned long long *c = &root[p][0];
      if ((uint32_t)c[0]) {
        b.n = (uint32_t)c[0], b.st = (long long)c[1];
        for (int i = 0; i < 3; ++i) b.s[i] = (long long)c[2 + i];
        for (int i = 0; i < 6; ++i) b.ss[i] = (long long)c[5 + i];
        b.tmin_inv = c[11], b.tmax_p1 = c[12];
        if (fx_starts(A, kFxTMax - b.tmin_inv, prev_p1, why_gap)) {
          ++root_ncl;
          closing = cur.n != 0u;
        }
        prev_p1 = b.tmax_p1;
      }
    }
    push_job(closing, cur, ord, owner);
    if (closing) {
      ++ord;
      fx_zero(cur);
    }
    if (b.n) fx_acc(cur, b);
  }
  push_job(root_ncl > 1u, cur, ord, owner);
  return root_ncl;
}

// ---- node tests (InitOctoTree cc:129-138, CutOctoTree cc:170-183) of the children (tot: a child's sums, ncl: its temporal
//      clusters) and the emission of the plane nodes with ONE temporal cluster: the cluster's sums are the node's, so is its PCA
//      (cc:32-64).  Out: rt = the root node (LEVEL 1: all children), parent_live, split = the group's tested non-plane children
//      (LEVEL 1 with a layer 2).  Returns the pending emission: its bucket entry is stored after the root's test (the atomic's
//      round trip runs beside it).  s_flag[lane]: the child is a plane with several temporal clusters, its jobs are emitted ----
template <int LEVEL>
__device__ __forceinline__ FxEmit fx_test_children(const FxArgs &A, bool have_parent, const FxPart &tot, uint32_t ncl, uint32_t key, uint32_t o1p, int kx,
                                                   int ky, int kz, const double *cc, float q0, uint32_t wsub, int why_slots, uint8_t *s_flag,
                                                   uint32_t *s_gkey, uint32_t *s_go1p, FxPart &rt, bool &parent_live, uint32_t &split) {
  const ExParams &P = A.P;
  const int lane = threadIdx.x, g = lane >> 3, gl = lane & 7;
  fx_zero(rt);
  if (LEVEL == 1) {
    rt = tot;
    fx_gsum8(rt);
  }
  parent_live = LEVEL == 1 ? (have_parent && (int)rt.n > P.min_points) : have_parent;  // nothing exists below an untested root
  const bool children_exist = LEVEL == 1 ? (P.max_layer >= 1) : true;
  const bool tested = parent_live && children_exist && (int)tot.n > P.min_points && !(WC_DBG(P, 256));
  // (the slots of the nodes with ONE temporal cluster are requested before the PCA that decides whether they are planes)
  const bool early = tested && ncl == 1u && (int)tot.n >= P.cluster_min;
  unsigned long long early_m;
  const uint32_t early_b = fx_slots_issue(A, wsub, early, early_m);
  FxPca pc;
  pc.near = false;
  if (tested) {
    fx_pca(A, tot, cc, pc);
    if (pc.near) fx_fallback(A.status, 13);
  }
  const bool plane = tested && (pc.r.ev[0] < P.thr) && (pc.r.like > P.min_like);  // cc:106-111
  split = (LEVEL == 1 && P.max_layer >= 2) ? ((uint32_t)(__ballot(tested && !plane) >> (g * 8)) & 0xFFu) : 0u;
  FxEmit pend;
  pend.on = false, pend.entry = 0, pend.bkt = 0, pend.r = 0, pend.rank = 0, pend.lead = lane;
  {
    const bool want = plane && ncl == 1u && (int)tot.n >= P.cluster_min && !(pc.r.ev[0] > P.thr || pc.r.like < P.min_like);
    const uint32_t sl = fx_slots_finish(A, wsub, early, early_m, early_b, why_slots);
    if (want && sl != 0xFFFFFFFFu) {
      if (LEVEL == 1)
        pend = fx_emit_begin(A, pc.r, sl, 1, (uint32_t)gl, 0u, 0u, kx, ky, kz, q0);
      else
        pend = fx_emit_begin(A, pc.r, sl, 2, o1p, (uint32_t)gl, 0u, kx, ky, kz, q0);
    }
  }
  s_flag[lane] = (plane && ncl > 1u && !(WC_DBG(P, 128))) ? 1 : 0;
  if (gl == 0) s_gkey[g] = key, s_go1p[g] = o1p, s_flag[64 + g] = 0;
  return pend;
}

// ---- the root node (LEVEL 1; Q4: a plane root emits AND its children are tested): lane 0 of the group.  root_ncl_of(rpl), a
//      WAVE-UNIFORM call, gives the number of temporal clusters of the lanes whose root is a plane ----
template <class RootNcl>
__device__ __forceinline__ void fx_test_root(const FxArgs &A, bool parent_live, const FxPart &rt, const double *cc, int kx, int ky, int kz, float q0,
                                             uint32_t wsub, int why_slots, uint8_t *s_flag, RootNcl root_ncl_of) {
  const ExParams &P = A.P;
  if (!__ballot(parent_live)) return;
  const int g = threadIdx.x >> 3, gl = threadIdx.x & 7;
  // (roots that provably are no planes - fx_surely_not_plane - skip the eigen-decomposition; a wavefront whose roots all are skips it
  // as a whole)
  const bool rtest = parent_live && gl == 0 && !fx_surely_not_plane(A, rt, cc);
  FxPca rp;
  rp.near = false;
  rp.r.ev[0] = 1e300, rp.r.like = 0.0;
  if (rtest) {
    fx_pca(A, rt, cc, rp);
    if (rp.near) fx_fallback(A.status, 14);
  }
  const bool rpl = rtest && (rp.r.ev[0] < P.thr) && (rp.r.like > P.min_like);
  const uint32_t root_ncl = root_ncl_of(rpl);
  if (rpl && root_ncl > 1u && !(WC_DBG(P, 1024))) s_flag[64 + g] = 1;
  const bool want = rpl && root_ncl == 1u && (int)rt.n >= P.cluster_min && !(rp.r.ev[0] > P.thr || rp.r.like < P.min_like);
  const uint32_t sl = fx_take_slots(A, wsub, want, why_slots);
  if (want && sl != 0xFFFFFFFFu) fx_emit(A, rp.r, sl, 0, 0u, 0u, 0u, kx, ky, kz, q0);
}

// ---- one job per lane (want): a cluster of a plane node with several of them.  PCA, cluster gates (cc:33, :54), emission under
//      the owner's identity (owner: lane of the child, 64 + group for a root; s_gkey / s_go1p: the groups' keys and octants) ----
template <int LEVEL>
__device__ __forceinline__ void fx_run_job(const FxArgs &A, bool want, uint32_t owner, const FxPart &cl, uint32_t ordv, int k0x, int k0y, int k0z,
                                           float q0, uint32_t wsub, const FxWhy &why, const uint32_t *s_gkey, const uint32_t *s_go1p) {
  const ExParams &P = A.P;
  const uint32_t og = owner < 64u ? owner >> 3 : owner - 64u;
  int jx, jy, jz;
  double jc[3];
  fx_key_voxel(P, s_gkey[og], k0x, k0y, k0z, jx, jy, jz, jc);
  FxPca cp;
  cp.near = false;
  if (want) {
    fx_pca(A, cl, jc, cp);
    if (cp.near) {
      fx_fallback(A.status, 15);
      if (why.job_which >= 0) fx_fallback(A.status, why.job_which + cp.which);
    }
    want = !(cp.r.ev[0] > P.thr || cp.r.like < P.min_like);
  }
  const uint32_t sl = fx_take_slots(A, wsub, want, why.slots);
  if (want && sl != 0xFFFFFFFFu) {
    if (owner >= 64u)
      fx_emit(A, cp.r, sl, 0, 0u, 0u, ordv, jx, jy, jz, q0);
    else if (LEVEL == 1)
      fx_emit(A, cp.r, sl, 1, owner & 7u, 0u, ordv, jx, jy, jz, q0);
    else
      fx_emit(A, cp.r, sl, 2, s_go1p[og], owner & 7u, ordv, jx, jy, jz, q0);
  }
}

// ---- LEVEL 1: queue the tested layer-1 nodes that are not planes (split) for the layer-2 pass (cc:175-182), one atomic per
//      wavefront for the eight groups' demands.  Returns whether this root keeps its header and hash entry for that pass ----
__device__ __forceinline__ bool fx_queue_layer2(const FxArgs &A, bool have_parent, uint32_t split, uint32_t pidx, uint32_t key, unsigned long long *blk,
                                                uint32_t wsub) {
  const int lane = threadIdx.x, g = lane >> 3, gl = lane & 7;
  const uint32_t nq = (uint32_t)__popc(split);
  uint32_t dem = (gl == 0 && have_parent) ? nq : 0u, pre = dem;
  for (int d = 8; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(pre, d);
    if (lane >= d) pre += o;
  }
  const uint32_t wave_total = (uint32_t)__shfl((int)pre, 56);
  uint32_t base_ = 0;
  if (wave_total) {
    if (lane == 0) base_ = atomicAdd(fx_cnt(A, kFxStNodes2, wsub), wave_total);
    base_ = (uint32_t)__shfl((int)base_, 0);
  }
  const uint32_t gbase = (uint32_t)__shfl((int)(base_ + pre - dem), g * 8);  // this group's first local index
  bool queued = false;
  if (have_parent && nq) {
    if (gbase + nq > A.mq_per) {
      fx_fallback(A.status, 16);
    } else {
      const uint32_t first = wsub * A.mq_per + gbase;
      queued = true;
      if (gl == 0) {
        uint32_t *w32 = (uint32_t *)blk;
        w32[12] = split;
        w32[13] = first;
      }
      if ((split >> gl) & 1u) {
        const uint32_t qn = first + (uint32_t)__popc(split & ((1u << gl) - 1u));
        uint32_t *q32 = (uint32_t *)(A.blk2 + (size_t)qn * kFxBlockW);
        const bool first_child = (split & ((1u << gl) - 1u)) == 0u;  // this node's group cleans the root's entries after the layer-2 pass
        q32[0] = pidx | ((uint32_t)gl << 28) | (first_child ? 0x80000000u : 0u);
        q32[1] = key + 1u;
      }
    }
  }
  return queued;
}

// ---- the tables are zero at rest: the list heads of this lane's child; the header and the root's hash entry (lane 0 of the group).
//      A root with queued layer-1 nodes keeps header and hash entry for the layer-2 pass (k_fx_acc<2> looks the root up and reads
//      the split mask); the group of its first queued node clears them afterwards ----
__device__ __forceinline__ void fx_clear_heads(unsigned long long *blk) {
  uint4 *hz = (uint4 *)(blk + kFxHdrW) + (threadIdx.x & 7) * 4;
  hz[0] = hz[1] = hz[2] = hz[3] = make_uint4(0u, 0u, 0u, 0u);
}
template <int LEVEL>
__device__ __forceinline__ void fx_clear_header(const FxArgs &A, unsigned long long *blk, uint32_t pidx, bool queued) {
  uint32_t *w32 = (uint32_t *)blk;
  if (LEVEL == 1) {
    if (!queued) {  // nothing queued (or the queue was full: flagged); (reading w32[12] back here cost a round trip)
      w32[2] = 0u;
      A.rkey[pidx] = 0u;
    }
  } else {
    const uint32_t ro = w32[0];
    w32[0] = w32[1] = w32[2] = 0u;
    if (ro & 0x80000000u) {
      const uint32_t rslot = ro & 0xFFFFFFFu;
      uint32_t *r32 = (uint32_t *)(A.blk + (size_t)rslot * kFxBlockW);
      r32[2] = r32[12] = r32[13] = 0u;
      A.rkey[rslot] = 0u;
    }
  }
}

// ---- the node stage in ONE launch: walk, tests, jobs, layer-2 queue and clean-up of eight parents per wavefront, kept in registers
//      from the walk to the tests ----
constexpr FxWhy kFxWhyNodes = {7, 8, 9, 10, 11, 12, -1};
template <int LEVEL>
__global__ void __launch_bounds__(64) k_fx_nodes(FxArgs A) {
  __shared__ uint32_t s_heads[64][kFxSlots + 1];          // the 16 list heads of every lane's child, in time order
  __shared__ unsigned long long s_root[8][kFxSlots][13];  // LEVEL 1: the time bins of the eight root nodes of the wavefront
  __shared__ uint8_t s_jown[kFxJobCap];  // owner of every job: lane of the child, 64 + group for a root
  __shared__ uint8_t s_flag[72];         // owner is a plane with several temporal clusters: its jobs are emitted
  __shared__ uint32_t s_gkey[8], s_go1p[8];
  const ExParams &P = A.P;
  const int lane = threadIdx.x, g = lane >> 3, gl = lane & 7;
  const uint32_t bank = LEVEL == 1 ? kFxStRoots : kFxStNodes2;
  const uint32_t per = LEVEL == 1 ? A.mr_per : A.mq_per;
  // The parents sit in kFxSub dense sub-lists (one counter each).  Two ways to hand them out:
  //  - small sweeps (one round of wavefronts; A.static_map): wavefront b takes sub-list b mod kFxSub, eight entries at a time.
  //    Which entries does not depend on the counters, so the entry (-> hash slot) is requested together with the one counter the
  //    wavefront needs: one dependent round trip less (~2 k of the 28 k clocks of the wavefront's chain);
  //  - large clouds: the sub-lists back to back, eight entries per wavefront (all sixteen counters first).  A sub-list is in
  //    creation = time order; with the static hand-out the wavefronts resident at one time work on one stretch of the cloud and
  //    their surfels land in the same few time buckets of the slot order (same-address atomics: 128 -> 197 us at 10 M points).
  const bool stat = A.static_map != 0u;
  const uint32_t sj = blockIdx.x & (kFxSub - 1);
  const uint32_t nwj = (gridDim.x - sj + kFxSub - 1) / kFxSub;  // wavefronts of this sub-list (static hand-out)
  uint32_t total = 0, cnts[kFxSub], cnt_j = 0;
  if (stat) {
    cnt_j = min(*fx_cnt(A, bank, (int)sj), per);
  } else {
#pragma unroll
    for (int j = 0; j < kFxSub; ++j) {
      cnts[j] = min(*fx_cnt(A, bank, j), per);
      total += cnts[j];
    }
  }
  double x0, y0, z0;
  ex_origin(A.pts, x0, y0, z0);
  const int k0x = vox(x0, P.vs), k0y = vox(y0, P.vs), k0z = vox(z0, P.vs);
  const float q0 = P.vs_f / 4;
  const uint32_t wsub = blockIdx.x & (kFxSub - 1);
  if (WC_DBG(P, 2048)) return;
  for (uint32_t it = 0;; ++it) {
    uint32_t pidx = 0;  // block index of this group's parent
    bool have_parent;
    if (stat) {
      const uint32_t chunk = blockIdx.x / kFxSub + it * nwj;
      if (chunk * 8u >= per) break;
      const uint32_t local = chunk * 8u + (uint32_t)g;
      pidx = sj * per + min(local, per - 1u);
      if (LEVEL == 1) {  // dense list entry -> hash slot = block index (an entry behind the counter is stale: masked, never used)
        pidx = A.rlist[pidx] & A.tr_mask;
        asm volatile("" : "+v"(pidx));  // (requested BEFORE the counter is looked at)
      }
      if (chunk * 8u >= cnt_j) break;
      have_parent = local < cnt_j;
    } else {
      const uint32_t w0 = (blockIdx.x + it * gridDim.x) * 8u;
      if (w0 >= total) break;
      const uint32_t gi = w0 + (uint32_t)g;
      have_parent = gi < total;
      pidx = fx_dense_parent<LEVEL>(A, cnts, per, gi, have_parent);
    }
    unsigned long long *blk = (LEVEL == 1 ? A.blk : A.blk2) + (size_t)pidx * kFxBlockW;
    uint32_t key, o1p, minbin;
    fx_parent_header<LEVEL>(A, blk, pidx, have_parent, key, o1p, minbin);
    int kx, ky, kz;
    double cc[3];
    fx_key_voxel(P, key, k0x, k0y, k0z, kx, ky, kz, cc);
    const uint32_t occ = fx_load_heads(blk, have_parent, minbin, s_heads[lane]);
    uint32_t jcnt = 0;  // jobs of this wavefront (uniform)
    // no node of the wavefront has more than one time bin (a sweep with run structure): a node's total IS its bin, and the
    // root's bins are only summed (below) if a root turns out to be a plane
    const bool one_bin = __ballot((occ & (occ - 1u)) != 0u) == 0ull;
    if (LEVEL == 1 && !one_bin) {  // the root node's time bins (all children together), summed in LDS while the children walk theirs
      for (int i = lane; i < 8 * kFxSlots * 13; i += 64) (&s_root[0][0][0])[i] = 0ull;
      __builtin_amdgcn_wave_barrier();
    }
    unsigned long long *jb = A.jobs + (size_t)blockIdx.x * kFxJobCap * kFxJobW;
    auto push_job = [&](bool closing, const FxPart &cl, uint32_t ordv, uint32_t owner) {  // (the owner in LDS too: the job loop loads only the jobs it runs)
      const uint32_t pos = fx_push_job(A, jb, jcnt, closing, cl, ordv, owner, kFxWhyNodes.jobs);
      if (pos < (uint32_t)kFxJobCap) s_jown[pos] = (uint8_t)owner;
    };
    FxPart tot;
    uint32_t ncl;
    fx_walk_node<LEVEL, kFxChains>(A, occ, minbin, s_heads[lane], LEVEL == 1 && !one_bin, s_root[g], kFxWhyNodes, push_job, tot, ncl);
    __builtin_amdgcn_wave_barrier();
    FxPart rt;
    bool parent_live;
    uint32_t split;
    const FxEmit pend = fx_test_children<LEVEL>(A, have_parent, tot, ncl, key, o1p, kx, ky, kz, cc, q0, wsub, kFxWhyNodes.slots, s_flag, s_gkey, s_go1p,
                                                rt, parent_live, split);
    if (LEVEL == 1) {
      fx_test_root(A, parent_live, rt, cc, kx, ky, kz, q0, wsub, kFxWhyNodes.slots, s_flag, [&](bool rpl) -> uint32_t {
        if (!__ballot(rpl)) return 0u;
        if (one_bin) {  // the root's bins were not summed during the walk: each child's one bin is its total
          for (int i = lane; i < 8 * kFxSlots * 13; i += 64) (&s_root[0][0][0])[i] = 0ull;
          __builtin_amdgcn_wave_barrier();
          const bool grp = ((__ballot(rpl) >> (g * 8)) & 0xFFull) != 0ull;
          if (grp && tot.n) fx_add_cell(&s_root[g][__ffs((int)occ) - 1][0], tot);
          __builtin_amdgcn_wave_barrier();
        }
        return fx_root_clusters(A, rpl, s_root[g], kFxWhyNodes.gap, push_job);
      });
    }
    fx_emit_end(A, pend);
    // ---- the jobs, one lane each ----
    if (jcnt) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the job stores of this wavefront are in L2
    __builtin_amdgcn_wave_barrier();
    for (uint32_t r0 = 0; r0 < min(jcnt, (uint32_t)kFxJobCap); r0 += 64u) {
      const uint32_t ji = r0 + (uint32_t)lane;
      bool want = ji < min(jcnt, (uint32_t)kFxJobCap);
      const uint32_t owner = want ? s_jown[ji] : 0u;
      want = want && s_flag[owner] != 0;
      if (!__ballot(want)) continue;
      FxPart cl;
      fx_zero(cl);
      uint32_t ordv = 0;
      if (want) {  // (agent-scope loads: L2, where the stores went - this CU's L1 may hold the bytes of an earlier round)
        const unsigned long long *o = jb + (size_t)ji * kFxJobW;
        unsigned long long w[11];
#pragma unroll
        for (int i = 0; i < 11; ++i) w[i] = __hip_atomic_load(&o[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cl.n = (uint32_t)w[0], ordv = (uint32_t)(w[0] >> 32), cl.st = (long long)w[1];
        for (int i = 0; i < 3; ++i) cl.s[i] = (long long)w[2 + i];
        for (int i = 0; i < 6; ++i) cl.ss[i] = (long long)w[5 + i];
      }
      fx_run_job<LEVEL>(A, want, owner, cl, ordv, k0x, k0y, k0z, q0, wsub, kFxWhyNodes, s_gkey, s_go1p);
    }
    __builtin_amdgcn_wave_barrier();
    const bool queued = LEVEL == 1 && fx_queue_layer2(A, have_parent, split, pidx, key, blk, wsub);
    if (have_parent && !(WC_DBG(P, 8192))) {
      fx_clear_heads(blk);
      if (gl == 0) fx_clear_header<LEVEL>(A, blk, pidx, queued);
    }
  }
}
