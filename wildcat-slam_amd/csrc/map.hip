// map.hip — device-resident voxel-downsampled point map: the reference's DownSamplingVoxel (src/odometry/surfel_extraction.cc:228-261,
// every occupied voxel of side `voxel_size` replaced by the centroid of its points) applied to the union of every cloud inserted so
// far - the accumulated map the reference's RViz builds from /scan_in_imu_frame (lidar_odometry.cc:584-595).
//
// Table (one per wc_map): open addressing, linear probing, a power-of-two number of slots.
//   keys[cap]     u64 packed voxel key (21 bits per axis, offset 2^20: ascending packed key = ascending (kx, ky, kz)); ~0 = empty,
//                 ~0 - 1 = a tombstone: a removed voxel, a foreign key to every probe and skipped by every pass over the slots
//   pay[cap][4]   i64 moments of the voxel's points: sum of q = round((p - r) * 2^32) per axis, count
// r is the voxel centre rounded to 1/1024 m, a function of the key alone, so every point's q is a deterministic function of the point:
// integer addition is associative, and the map is bit-identical however the same points are split across calls, ordered or
// scheduled.  |p - r| <= v / 2 + 2^-11 <= 2.0005 m, so a voxel holds up to 2^30 points before a sum could overflow.
//   mom[cap][9]   i64, only in a map created with WC_MAP_MOMENTS: with u = (q + 2^15) >> 16 (arithmetic shift: q rounded to 2^-16 m, a
//                 function of the point alone) the sums of u per axis (3 words) and of u_a u_b for ab = xx, xy, xz, yy, yz, zz (6 words).
//                 |u| < 2^17.001, every product < 2^34.01: such a voxel holds up to 2^28 points before a second moment could overflow.
//                 Integer sums again: the moments are as order independent as the centroids.  pay[] is what it is in a plain map.
// Kernels (all on the ctx's stream):
//   k_map_insert    tiles of 512 consecutive points per workgroup: each lane folds its 2 points into a run while the voxel stays the
//                   same, the tile's voxels are pre-aggregated in an LDS hash (1024 slots, at most half full), then ONE global probe
//                   and four integer atomic adds per distinct voxel of the tile; counters once per workgroup.  <true, .>: the nine
//                   moment sums ride along (nine more LDS words per hash slot, thirteen global atomics per distinct voxel)
//   k_map_rehash<SEL>  growth, crop: the occupied slots of the old table that a selector (map_sel_all, map_sel_box; map_sel_carve for
//                   the count) selects into the new one (distinct keys: plain stores of the payload) - map_replace_table
//   k_map_compact   export: occupied slots -> (key, slot) pairs (LDS staging, one atomic per workgroup); rocPRIM radix sort by key
//   k_map_centroids export: centroid = r + sum / (count * 2^32) in fp64, rounded once to float; count; key (optional)
//   k_map_nearest   query: one lane per query; the first-slot key loads of the 27 voxels around the query's own are issued nine at a
//                   time before any is examined, payload loads and divisions only for the occupied ones; read-only probes, no CAS
//   k_map_knn<KMAX, REACH>  k nearest within a radius: one lane per query; the 27 or 125 voxels around it in ascending key order, the
//                   first-slot key loads of nine (an x plane) or five (a z row) in flight together, read-only chains; a sorted list of
//                   KMAX (d2, slot) entries in registers, every index a compile-time constant; k records per query, the count of
//                   accepted voxels uncapped: wc_map_knn
//   k_map_count<SEL>  the selected voxels and their points, counted per workgroup: a crop's kept ones (then k_map_rehash<map_sel_box>),
//                   a carve's seen-through ones
//   k_map_surfels   surfel export: one lane per sorted voxel: map_plane_of (exact 128-bit covariance numerator, fx_eig3) -> wc_map_surfel
//   k_map_nearest<true>  plane query: the same search, then map_plane_of for the winning voxel only -> wc_map_plane_hit
//   k_map_linearize<ONE> / k_map_lin_reduce  registration: the plane query behind a pose, reduced to the point-to-plane normal equations
//                   in a fixed order (tiles of 256 points, then levels of 32 partials, one launch each), for K poses of one point set
//                   in one launch chain with (hypothesis, tile) pairs as work items; <true>: one pose, in the kernel arguments.  One
//                   host core (lin_core) under wc_map_linearize, wc_map_align, their pyramid and their _batch forms
//   k_map_linearize_ct  registration of a stamped sweep between two poses: every point through the pose interpolated at its stamp
//                   (map_move_ct), the same search, 76 sums in the same order, k_map_lin_reduce<80, 76>: wc_map_linearize_ct,
//                   wc_map_align_ct
//   k_map_score_batch  occupancy score of K poses of one point set: a tile of 256 points in registers walks a block of hypotheses, one
//                   read-only probe chain per (point, pose), eight hypotheses' first-slot key loads in flight; counts by ballot, LDS and one
//                   32-bit atomic add per workgroup, hypothesis and count: wc_map_score_batch
//   k_map_carve    carving: one lane per ray from the call's origin to a point: the end voxel's word gets its mark, then the counted voxel
//                   walk, eight steps ahead of the probes: keys, hashes and shell tests of a batch, its first-slot key loads issued
//                   together, then the chains (read-only) and one no-return atomic add per occupied voxel seen through;
//                   k_map_count<map_sel_carve> then counts the voxels the words select: wc_map_carve (which reports and does not remove)
//   k_map_erase<SEL>  k_map_count's pass that also turns the selected slots' keys into tombstones and takes them off the map's counters:
//                   wc_map_carve_remove
//   k_map_remove_keys  one lane per voxel index: probe, then a CAS of the key word to the tombstone: wc_map_remove_keys
//   k_map_raycast  ray casting: the carve's ray and walk, read-only: one lane per ray, its M + 1 positions eight at a time - keys, hashes and
//                   tested-flags of a batch, its first-slot key loads issued together, then the chains in ascending order up to the first
//                   voxel with enough points - and one 48-byte wc_map_ray_hit per ray; no atomics but its four counters': wc_map_raycast
//   k_map_cc_index / _link / _flatten / _clear / _stats / _select / _erase  connected components of the occupied voxels: a per-slot index
//                   word, lock-free union-find over the export order (every access to the parent array an agent-scope atomic, every
//                   loop bounded), pointer jumping in a launch of its own, a rocPRIM scan of the root flags, integer atomics per component;
//                   the last one writes tombstones: wc_map_components, wc_map_remove_small
//   k_map_state    state export: one lane per sorted voxel: the slot's integer sums themselves -> wc_map_voxel (+ nine moment words)
//   k_map_absorb   state records added back by key (map_slot, then four / thirteen no-return atomic adds): wc_map_absorb
//   k_map_merge    the same for every occupied slot of another map's table: wc_map_merge
//   k_map_coarsen  the merge's pass with the key divided and the sums re-based to the coarse voxel's reference point in registers: the
//                   new map of wc_map_coarsen, factor^3 voxels to one
// Shared pieces: map_voxel_of (the voxel-index rule, host and device), map_find_from (the read-only probe chain), block_count (a
// workgroup's counters), map_points_ok (a wc_points argument), map_replace_table (new table, rehash, free the old one), map_ray_of /
// map_ray_begin / map_ray_step (a ray's setup and the step rule of its voxel walk: the carve and the ray cast), map_move (a point through
// a pose: the registration and the score)
// Growth policy: before an insert of n points the host takes an upper bound B of the occupied slots (the exact count of the last
// completed insert's read-back plus every point inserted after it); when 2 (B + n) > cap the table is rehashed into the smallest power
// of two >= 2 (B + n) slots.  The table is therefore at most half full at every probe, and an insert never runs out of room.
// Tombstones hold slots: map_room.h takes the decision with them counted, and a table they alone have filled is replaced by a fresh
// one of the same size (a purge).  A replacement of any kind drops them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "ctx.h"
#include "dmath.h"
#include "map_room.h"

struct wc_map {
  wc_ctx *ctx = nullptr;
  double voxel = 0;
  uint64_t cap = 0;                  // slots (power of two)
  unsigned long long *keys = nullptr;
  long long *pay = nullptr;          // 4 per slot: sum qx, qy, qz, count
  long long *mom = nullptr;          // WC_MAP_MOMENTS: 9 per slot: sum ux, uy, uz, uxux, uxuy, uxuz, uyuy, uyuz, uzuz; else NULL
  uint32_t flags = 0;                // wc_map_create_ex's
  unsigned long long *ctr = nullptr; // device counters, each on a 128-byte line of its own (see kCtr*)
  unsigned long long *h_ctr = nullptr;  // pinned copy of the counters, written after every insert
  hipEvent_t ev_ctr = nullptr;       // recorded after that copy
  bool ctr_pending = false;          // an insert's copy has been enqueued and not yet taken into occ_known
  uint64_t occ_known = 0;            // occupied slots at the last completed read-back ...
  uint64_t pts_since = 0;            // ... plus the points of every insert after it bound the occupied slots
  uint64_t pts_after_copy = 0;       // points of the inserts enqueued behind the pending copy
  uint64_t growths = 0;
  uint64_t tombs = 0;                // tombstones in the table: exact, the removal calls wait and know what they removed
  uint64_t purges = 0;               // replacements into a table of the same size, made to drop tombstones
  int cus = 256;
  wc_buf b_pairs[4], b_tmp, b_cnt;   // export scratch: keys in / out, slot indices in / out; rocPRIM temporary; compaction counter
  wc_buf b_lin;                      // lin_core: K hypotheses' tile partials and every level of their reduction, then the K final partials
  unsigned long long *h_lin = nullptr;  // ... and the pinned landing place of those K final partials: it holds h_lin_cap, grown on demand
  uint64_t h_lin_cap = 0;
  wc_buf b_pose;                     // lin_core with K > 1: the poses, K x 12 doubles (one pose travels in the kernel arguments) ...
  double *h_pose = nullptr;          // ... and the pinned block they are uploaded from: h_lin_cap hypotheses once that exceeds 1
  wc_buf b_carve;                    // wc_map_carve: its five counter lines, then one u32 word per slot (first use, grown with the table)
  unsigned long long *h_carve = nullptr;  // ... and the pinned landing place of the counters (first use)
  wc_buf b_cast;                     // wc_map_raycast: its four counter lines (first use); nothing another call reads or writes
  unsigned long long *h_cast = nullptr;  // ... and their pinned landing place (first use)
  wc_buf b_score;                    // wc_map_score_batch: K x 16 bytes of counts, then the K x 12 doubles of the poses; its own scratch
  unsigned char *h_score = nullptr;  // ... and the pinned block of the same layout, grown on demand: it holds h_score_cap hypotheses
  uint64_t h_score_cap = 0;
  wc_buf b_ct;                       // wc_map_linearize_ct: the tile partials (80 words each) and every level of their reduction; its own scratch
  unsigned long long *h_ct = nullptr;  // ... and the pinned landing place of the final partial, 640 bytes (first use)
  wc_buf b_cc_idx;                   // wc_map_components / wc_map_remove_small: one u32 word per slot, slot -> export index (first use, grown with the table)
  wc_buf b_cc;                       // ... their counter lines, then four u32 arrays per export entry: parent, root, root flag, component number
  wc_buf b_cc_comps;                 // ... the C records, then one u32 selection word per component
  wc_buf b_cc_tmp;                   // ... rocPRIM's temporary of the scan; all four are this feature's own scratch
  unsigned long long *h_cc = nullptr;  // ... and the pinned landing place of the counters (first use)
};

namespace {

#include "fx_eig3.h"

constexpr int kMapThreads = 256;
constexpr int kMapPts = 2;                         // consecutive points per lane (a tile: kMapThreads times as many)
constexpr int kMapMom = 9;                         // moment words per slot of a WC_MAP_MOMENTS map
constexpr int kMapMomPts = 1;                      // points per lane of the moments insert (the alternative form: DESIGN, "Map surfels")
constexpr unsigned long long kMapEmpty = ~0ull;
constexpr unsigned long long kMapTomb = ~0ull - 1;  // a removed voxel: no packed key (63 bits), not empty; a slot is occupied iff key < kMapTomb
constexpr double kMapUnit = 4294967296.0;          // fixed-point unit: 2^-32 m
constexpr double kMapKeyLim = 1048576.0;           // |k| < 2^20
constexpr int kMapKeyOff = 1 << 20;
constexpr int kCtrOcc = 0, kCtrPts = 16, kCtrRej = 32, kCtrRejCall = 48, kCtrLost = 56;  // u64 word of each counter
constexpr int kCtrFound = 64, kCtrKeepVox = 80, kCtrKeepPts = 96;                        // query hits; a crop's kept voxels, points
constexpr int kCtrRmVox = 112, kCtrRmPts = 128, kCtrRmNone = 144;                        // wc_map_remove_keys: voxels, points, keys that removed nothing
constexpr int kCtrMvVox = 160, kCtrMvPts = 176, kCtrMvRejVox = 192, kCtrMvRejPts = 208, kCtrMvEnd = 224;  // wc_map_merge_moved: this call's four counts
constexpr int kCtrKnnSome = 224, kCtrKnnRec = 240, kCtrKnnWithin = 256, kCtrWords = 272;  // wc_map_knn: queries with a neighbour, records, sum of within
constexpr int kNearThreads = 256;
constexpr int kCompactChunk = 2048;                // slots per workgroup of k_map_compact
constexpr int kCarveThreads = 256;
constexpr int kCarveBatch = 8;                     // steps of a ray whose first-slot key loads are in flight together
constexpr unsigned kCarveEnd = 0x80000000u;        // a slot's word: bit 31 = an end voxel of this call; low 31 bits = through(k)
constexpr int kCastThreads = 256;
constexpr int kCastBatch = 8;                      // positions of a ray whose first-slot key loads are in flight together
constexpr int kCastCast = 0, kCastSkip = 16, kCastHits = 32, kCastTested = 48, kCastCtrWords = 64;  // u64 word of each of wc_map_raycast's counters
constexpr int kCarveUsed = 0, kCarveSkip = 16, kCarveSteps = 32, kCarveSelVox = 48, kCarveSelPts = 64, kCarveCtrWords = 80;  // u64 word of each of wc_map_carve's counters

__device__ __forceinline__ unsigned long long map_hash(unsigned long long k) {  // splitmix64 finaliser
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return k;
}
// reference point of a voxel on the 2^-10 m grid: the voxel centre, rounded; a function of (k, v) alone
__host__ __device__ __forceinline__ double map_ref(int k, double v) { return rint(((double)k + 0.5) * v * 1024.0) * (1.0 / 1024.0); }
__device__ __forceinline__ int map_unpack(unsigned long long key, int axis) {
  return (int)((key >> (42 - 21 * axis)) & 0x1FFFFFull) - kMapKeyOff;
}
__device__ __forceinline__ unsigned long long map_pack(int kx, int ky, int kz) {
  return ((unsigned long long)(kx + kMapKeyOff) << 42) | ((unsigned long long)(ky + kMapKeyOff) << 21) | (unsigned long long)(kz + kMapKeyOff);
}
// one coordinate of a voxel's centroid from its exact integer sum s and its count c: the export and the query share this expression,
// so a hit's xyz is byte-equal to the exported centroid
__device__ __forceinline__ float map_centroid(int k, double v, long long s, double c) {
  return (float)(map_ref(k, v) + (double)s / (c * kMapUnit));
}
// a point's coordinate in the moments' unit, 2^-16 m: q rounded (arithmetic shift; ties up), a function of the point alone
__device__ __forceinline__ long long map_u(long long q) { return (q + 32768) >> 16; }
// the sum of a 64-lane wavefront in lane 0
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int o = 32; o; o >>= 1) x += __shfl_down(x, o);
  return x;
}
// N per-lane counts of a workgroup of THREADS lanes, each onto its counter: the sum over the wavefront, one LDS word per wavefront and
// count, thread 0 adds them, and one atomic per counter (each on a line of its own) when the sum is non-zero.  Integers: no order matters
template <int THREADS, class T, int N>
__device__ __forceinline__ void block_count(const T (&x)[N], unsigned long long *const (&ctr)[N]) {
  __shared__ T s_part[N][THREADS / 64];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const T w = wave_sum(x[c]);
    if ((threadIdx.x & 63) == 0) s_part[c][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
      T t = 0;
#pragma unroll
      for (int w = 0; w < THREADS / 64; ++w) t += s_part[c][w];
      if (t) atomicAdd(ctr[c], (unsigned long long)t);
    }
  }
}

// VoxelLoc (surfel_extraction.h:59-64): k = floor((double)p / v) per axis, true fp64 division.  false: the point has no voxel - NaN, inf
// and |k| >= 2^20 fail the strict compares - and k is 0 on every axis
__host__ __device__ __forceinline__ bool map_voxel_of(double x, double y, double z, double v, int &kx, int &ky, int &kz) {
  const double fx = floor(x / v), fy = floor(y / v), fz = floor(z / v);
  const bool ok = fx > -kMapKeyLim && fx < kMapKeyLim && fy > -kMapKeyLim && fy < kMapKeyLim && fz > -kMapKeyLim && fz < kMapKeyLim;
  kx = ok ? (int)fx : 0, ky = ok ? (int)fy : 0, kz = ok ? (int)fz : 0;
  return ok;
}

// one global probe: the slot of `key`, claimed if it is new (fresh += 1).  The table is at most half full, so the loop ends; the bound
// on its length only guards against a broken invariant (the key is then dropped and ctr[kCtrLost] counts it)
__device__ __forceinline__ unsigned long long map_slot(unsigned long long *keys, unsigned long long mask, unsigned long long key, unsigned &fresh) {
  unsigned long long h = map_hash(key) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    unsigned long long cur = keys[h];  // (a stale EMPTY is settled by the CAS; a key once written never changes during an insert)
    if (cur == kMapEmpty) {
      cur = atomicCAS(&keys[h], kMapEmpty, key);
      if (cur == kMapEmpty) {
        ++fresh;
        return h;
      }
    }
    if (cur == key) return h;
    h = (h + 1) & mask;
  }
  return kMapEmpty;
}
// the read-only probe chain of `key` from its first slot h, whose key c has been loaded: linear probing past foreign keys; true: h is the
// key's slot; false: the key is absent
__device__ __forceinline__ bool map_find_from(const unsigned long long *keys, unsigned long long mask, unsigned long long key,
                                              unsigned long long &h, unsigned long long c) {
  for (unsigned long long probe = 0; c != key && c != kMapEmpty && probe < mask; ++probe) {
    h = (h + 1) & mask;
    c = keys[h];
  }
  return c == key;
}

template <int LDS>
__device__ __forceinline__ unsigned lds_add(unsigned long long *lk, unsigned long long *ls, unsigned *lc, unsigned long long key,
                                            long long qx, long long qy, long long qz, unsigned n) {
  unsigned s = (unsigned)map_hash(key) & (LDS - 1);
  while (true) {
    unsigned long long cur = lk[s];
    if (cur == kMapEmpty) cur = atomicCAS(&lk[s], kMapEmpty, key);
    if (cur == kMapEmpty || cur == key) break;
    s = (s + 1) & (LDS - 1);
  }
  atomicAdd(&ls[s], (unsigned long long)qx);
  atomicAdd(&ls[LDS + s], (unsigned long long)qy);
  atomicAdd(&ls[2 * LDS + s], (unsigned long long)qz);
  atomicAdd(&lc[s], n);
  return s;
}
// the nine moment sums of a run into the LDS slot lds_add found (word w of slot s at lm[w * LDS + s], as ls)
template <int LDS>
__device__ __forceinline__ void lds_add_mom(unsigned long long *lm, unsigned s, const long long (&sm)[kMapMom]) {
#pragma unroll
  for (int w = 0; w < kMapMom; ++w) atomicAdd(&lm[w * LDS + s], (unsigned long long)sm[w]);
}

// MOM: the map holds moments (mom != NULL); PTS: consecutive points per lane (the plain map: kMapPts)
template <bool MOM, int PTS>
__global__ void __launch_bounds__(kMapThreads) k_map_insert(wc_points pts, double v, unsigned long long *keys, long long *pay, long long *mom,
                                                            unsigned long long mask, unsigned long long *ctr) {
  // (kMapTile: points per tile; kMapLds: LDS hash slots - a tile's voxels fill at most half of it)
  constexpr int kMapPts = PTS, kMapTile = kMapThreads * PTS, kMapLds = 2 * kMapTile;
  __shared__ unsigned long long lk[kMapLds];
  __shared__ unsigned long long ls[3 * kMapLds];
  __shared__ unsigned lc[kMapLds];
  __shared__ unsigned long long lm[MOM ? kMapMom * kMapLds : 1];
  __shared__ unsigned c_fresh, c_pts, c_rej;
  const int t = threadIdx.x;
  for (int s = t; s < kMapLds; s += kMapThreads) {
    lk[s] = kMapEmpty;
    ls[s] = ls[kMapLds + s] = ls[2 * kMapLds + s] = 0;
    lc[s] = 0;
    if constexpr (MOM) {
#pragma unroll
      for (int w = 0; w < kMapMom; ++w) lm[w * kMapLds + s] = 0;
    }
  }
  if (t == 0) c_fresh = c_pts = c_rej = 0;
  unsigned fresh = 0, n_ok = 0, n_rej = 0;
  const uint64_t tiles = (pts.n + kMapTile - 1) / kMapTile;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();
    // pass 1: the lane's consecutive points as runs of one voxel, each run into the LDS hash
    unsigned long long run_key = kMapEmpty;
    long long sx = 0, sy = 0, sz = 0;
    long long sm[kMapMom] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned rn = 0;
    const uint64_t i0 = tile * kMapTile + (uint64_t)t * kMapPts;
#pragma unroll
    for (int j = 0; j < kMapPts; ++j) {
      const uint64_t i = i0 + j;
      if (i >= pts.n) break;
      const float *f = (const float *)((const char *)pts.xyz + i * pts.xyz_stride);
      const double x = (double)f[0], y = (double)f[1], z = (double)f[2];
      int kx, ky, kz;
      if (!map_voxel_of(x, y, z, v, kx, ky, kz)) {
        ++n_rej;
        continue;
      }
      ++n_ok;
      const unsigned long long key = map_pack(kx, ky, kz);
      const long long qx = llrint((x - map_ref(kx, v)) * kMapUnit), qy = llrint((y - map_ref(ky, v)) * kMapUnit),
                      qz = llrint((z - map_ref(kz, v)) * kMapUnit);
      if (key != run_key) {
        if (rn) {
          const unsigned s = lds_add<kMapLds>(lk, ls, lc, run_key, sx, sy, sz, rn);
          if constexpr (MOM) lds_add_mom<kMapLds>(lm, s, sm);
        }
        run_key = key, sx = sy = sz = 0, rn = 0;
        if constexpr (MOM) {
#pragma unroll
          for (int w = 0; w < kMapMom; ++w) sm[w] = 0;
        }
      }
      sx += qx, sy += qy, sz += qz, ++rn;
      if constexpr (MOM) {
        const long long ux = map_u(qx), uy = map_u(qy), uz = map_u(qz);
        sm[0] += ux, sm[1] += uy, sm[2] += uz;
        sm[3] += ux * ux, sm[4] += ux * uy, sm[5] += ux * uz, sm[6] += uy * uy, sm[7] += uy * uz, sm[8] += uz * uz;
      }
    }
    if (rn) {
      const unsigned s = lds_add<kMapLds>(lk, ls, lc, run_key, sx, sy, sz, rn);
      if constexpr (MOM) lds_add_mom<kMapLds>(lm, s, sm);
    }
    __syncthreads();
    // pass 2: one global probe and four integer atomics per distinct voxel of the tile; the LDS hash is cleared behind it
    for (int s = t; s < kMapLds; s += kMapThreads) {
      const unsigned long long key = lk[s];
      if (key == kMapEmpty) continue;
      const unsigned long long h = map_slot(keys, mask, key, fresh);
      if (h != kMapEmpty) {
        unsigned long long *p = (unsigned long long *)pay + 4 * h;
        atomicAdd(p + 0, ls[s]);
        atomicAdd(p + 1, ls[kMapLds + s]);
        atomicAdd(p + 2, ls[2 * kMapLds + s]);
        atomicAdd(p + 3, (unsigned long long)lc[s]);
        if constexpr (MOM) {
          unsigned long long *pm = (unsigned long long *)mom + kMapMom * h;
#pragma unroll
          for (int w = 0; w < kMapMom; ++w) atomicAdd(pm + w, lm[w * kMapLds + s]);
        }
      } else {
        atomicAdd(ctr + kCtrLost, 1ull);
      }
      lk[s] = kMapEmpty;
      ls[s] = ls[kMapLds + s] = ls[2 * kMapLds + s] = 0;
      lc[s] = 0;
      if constexpr (MOM) {
#pragma unroll
        for (int w = 0; w < kMapMom; ++w) lm[w * kMapLds + s] = 0;
      }
    }
  }
  if (fresh) atomicAdd(&c_fresh, fresh);
  if (n_ok) atomicAdd(&c_pts, n_ok);
  if (n_rej) atomicAdd(&c_rej, n_rej);
  __syncthreads();
  if (t == 0) {
    if (c_fresh) atomicAdd(ctr + kCtrOcc, (unsigned long long)c_fresh);
    if (c_pts) atomicAdd(ctr + kCtrPts, (unsigned long long)c_pts);
    if (c_rej) {
      atomicAdd(ctr + kCtrRej, (unsigned long long)c_rej);
      atomicAdd(ctr + kCtrRejCall, (unsigned long long)c_rej);
    }
  }
}

// Selectors: a predicate on an occupied slot (its key, its index), passed by value to k_map_rehash (the slots that move) and k_map_count
// (the slots that are counted).  Every occupied slot (growth: no test is compiled)
struct map_sel_all {
  __device__ bool operator()(unsigned long long, uint64_t) const { return true; }
};
// an inclusive range of voxel indices per axis (wc_map_crop)
struct map_sel_box {
  int lo[3], hi[3];
  __device__ bool operator()(unsigned long long key, uint64_t) const {
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int k = map_unpack(key, a);
      in = in && k >= lo[a] && k <= hi[a];
    }
    return in;
  }
};
// what a carve's words select: at least min_rays rays saw through the voxel and no point of the call marked it (wc_map_carve)
struct map_sel_carve {
  const unsigned *words;
  unsigned min_rays;
  __device__ bool operator()(unsigned long long, uint64_t i) const {
    const unsigned w = words[i];
    return (w & kCarveEnd) == 0u && w >= min_rays;
  }
};

// the old table's occupied slots that `sel` selects into the new one (empty keys, zero payload); keys are distinct, so the payload is
// stored plainly.  omom / mom: NULL for a plain map
template <class SEL>
__global__ void __launch_bounds__(256) k_map_rehash(const unsigned long long *okeys, const long long *opay, const long long *omom, uint64_t ocap,
                                                    unsigned long long *keys, long long *pay, long long *mom, unsigned long long mask, SEL sel) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ocap) return;
  const unsigned long long key = okeys[i];
  if (key >= kMapTomb) return;  // (empty or a tombstone: tombstones never move, so every replacement purges them)
  if (!sel(key, i)) return;
  unsigned fresh = 0;
  const unsigned long long h = map_slot(keys, mask, key, fresh);
  if (h == kMapEmpty) return;  // (cannot happen: the new table has room for every old key)
  const longlong2 *src = (const longlong2 *)(opay + 4 * i);
  longlong2 *dst = (longlong2 *)(pay + 4 * h);
  dst[0] = src[0];
  dst[1] = src[1];
  if (omom) {  // (a WC_MAP_MOMENTS map: the nine moment words travel with the voxel)
#pragma unroll
    for (int w = 0; w < kMapMom; ++w) mom[kMapMom * h + w] = omom[kMapMom * i + w];
  }
}

// export, step 1: (key, slot) of every occupied slot, staged in LDS per chunk, one atomic per workgroup for its output range
__global__ void __launch_bounds__(256) k_map_compact(const unsigned long long *keys, uint64_t cap, unsigned long long *out_keys,
                                                     uint32_t *out_slots, uint64_t n_out, unsigned long long *d_cnt) {
  __shared__ unsigned long long sk[kCompactChunk];
  __shared__ uint32_t ss[kCompactChunk];
  __shared__ unsigned n_local;
  __shared__ unsigned long long base;
  if (threadIdx.x == 0) n_local = 0;
  __syncthreads();
  const uint64_t s0 = (uint64_t)blockIdx.x * kCompactChunk;
  for (int j = threadIdx.x; j < kCompactChunk; j += blockDim.x) {
    const uint64_t s = s0 + j;
    if (s >= cap) break;
    const unsigned long long key = keys[s];
    if (key >= kMapTomb) continue;
    const unsigned at = atomicAdd(&n_local, 1u);
    sk[at] = key;
    ss[at] = (uint32_t)s;
  }
  __syncthreads();
  if (threadIdx.x == 0) base = n_local ? atomicAdd(d_cnt, (unsigned long long)n_local) : 0;
  __syncthreads();
  for (unsigned j = threadIdx.x; j < n_local && base + j < n_out; j += blockDim.x) {
    out_keys[base + j] = sk[j];
    out_slots[base + j] = ss[j];
  }
}

// export, step 3: the sorted voxels' centroids - the reference's center / count (surfel_extraction.cc:258) from the exact integer
// sums, formed in fp64 and rounded to float once
__global__ void __launch_bounds__(256) k_map_centroids(const unsigned long long *skeys, const uint32_t *sslots, uint64_t n, const long long *pay,
                                                       double v, float *xyz, uint32_t *count, int32_t *keys_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = skeys[i];
  const long long *p = pay + 4 * (uint64_t)sslots[i];
  const double c = (double)p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int k = map_unpack(key, a);
    xyz[3 * i + a] = map_centroid(k, v, p[a], c);
    if (keys_out) keys_out[3 * i + a] = k;
  }
  count[i] = (uint32_t)p[3];
}

// ---- planes (WC_MAP_MOMENTS) ----------------------------------------------------------------------------------------------------
// a non-negative 128-bit integer rounded ONCE (to nearest, ties to even) to fp64.  The device has no library conversion for __int128:
// the top 64 bits of the normalised value, with every bit below them folded into bit 0 (eleven places under the rounding position, so it
// only breaks ties), go through the hardware's correctly rounded u64 conversion; the scaling by a power of two is exact
// (__host__ too: wc_map_move_state runs map_move_voxel without a GPU; the host has no __clzll, hi != 0 there)
__host__ __device__ __forceinline__ double map_u128_to_double(unsigned __int128 m) {
  const unsigned long long hi = (unsigned long long)(m >> 64), lo = (unsigned long long)m;
  if (hi == 0) return (double)lo;
#if defined(__HIP_DEVICE_COMPILE__)
  const int s = __clzll((long long)hi);
#else
  const int s = __builtin_clzll(hi);
#endif
  const unsigned __int128 n = m << s;
  const unsigned long long top = (unsigned long long)(n >> 64) | ((unsigned long long)n != 0 ? 1ull : 0ull);
  return ldexp((double)top, 64 - s);
}
// what wc_map_export_surfels and wc_map_nearest_plane both say about one voxel
struct map_plane {
  double cov[6], ev[3], nrm[3];
  unsigned plane;  // 1: count >= 3 and ev[2] > 0
};
// Population covariance of the voxel's quantised points from its count n and its nine moment words: exactly N_ab / (n^2 2^32) with the
// integer N_ab = n M_ab - U_a U_b (|N_ab| < 2^91: formed in 128 bits).  Roundings: one of the numerator (at most 1 ulp of the result:
// half an ulp of a number that may sit at the other end of its binade), one IEEE division by hi = fp64(n^2), and - n^2 has up to 56 bits
// - one of the quotient corrected for n^2 = hi + lo: the division's remainder r = fma(-q, hi, num) is exact, (r - q lo) / hi is the
// rest of num / (hi + lo) to second order.  Within 1.5 ulp plus second-order terms, under the 2 ulp the interface states; a plain
// fp64(N) / fp64(n^2) could reach 2.5 ulp for n > 2^26.  The power of two is exact.  Then fx_eig3 (closed form, Jacobi where its
// residual test refuses or the matrix is diagonal), and the sign rule: the normal's component of largest magnitude (the lowest axis
// on a tie) is positive.
__device__ __forceinline__ map_plane map_plane_of(long long count, const long long *mo) {
  map_plane r;
  const __int128 n = (__int128)count;
  const unsigned long long n2 = (unsigned long long)count * (unsigned long long)count;
  const double hi = (double)n2, lo = (double)(long long)(n2 - (unsigned long long)hi);
  const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const __int128 N = n * (__int128)mo[3 + e] - (__int128)mo[ia[e]] * (__int128)mo[ib[e]];
    const bool neg = N < 0;
    const double mag = map_u128_to_double(neg ? (unsigned __int128)(-N) : (unsigned __int128)N);
    const double num = neg ? -mag : mag, q = num / hi;
    r.cov[e] = (q + (fma(-q, hi, num) - q * lo) / hi) * (1.0 / 4294967296.0);
  }
  wc::M3 C, V;
  C.m[0][0] = r.cov[0], C.m[0][1] = C.m[1][0] = r.cov[1], C.m[0][2] = C.m[2][0] = r.cov[2];
  C.m[1][1] = r.cov[3], C.m[1][2] = C.m[2][1] = r.cov[4], C.m[2][2] = r.cov[5];
  bool closed = false;
  fx_eig3(C, r.ev, V, &closed);
  if (closed) {
    // fx_eig3 accepts its closed form at a residual of 1e-12 of the scale: enough for extraction, whose clusters of > 20 points are
    // plane-like, but a voxel of three nearly collinear points (lambda_1 << lambda_2) gets ev[0] from a cancelling sqrt(1 - x^2), some
    // 1e-13 of the scale off.  The interface promises 32 x 2^-53: the closed form stays only where |(C - ev[0] I) n| is at rounding
    // level, 8 x 2^-53 of the scale - an eigenvalue of a symmetric matrix lies within the residual of ev[0], and n within
    // residual / gap of its vector; the five or so ulps of rounding in the residual itself only send more voxels to the Jacobi iteration
    const double vx = V.m[0][0], vy = V.m[1][0], vz = V.m[2][0], e0 = r.ev[0];
    const double rx = (r.cov[0] - e0) * vx + r.cov[1] * vy + r.cov[2] * vz, ry = r.cov[1] * vx + (r.cov[3] - e0) * vy + r.cov[4] * vz,
                 rz = r.cov[2] * vx + r.cov[4] * vy + (r.cov[5] - e0) * vz;
    const double tol = 8.0 * 1.1102230246251565e-16 * fmax(fabs(r.ev[0]), fabs(r.ev[2]));
    if (!(rx * rx + ry * ry + rz * rz <= tol * tol)) wc::eig3_sym(C, r.ev, V);
  }
  double nx = V.m[0][0], ny = V.m[1][0], nz = V.m[2][0];
  const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
  const double lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
  if (lead < 0.0) nx = -nx, ny = -ny, nz = -nz;
  r.nrm[0] = nx, r.nrm[1] = ny, r.nrm[2] = nz;
  r.plane = (count >= 3 && r.ev[2] > 0.0) ? 1u : 0u;
  return r;
}

// surfel export, step 3: one lane per sorted voxel (the eigen-solve is a dependent chain; the export is not a per-sweep call)
__global__ void __launch_bounds__(256) k_map_surfels(const unsigned long long *skeys, const uint32_t *sslots, uint64_t n, const long long *pay,
                                                     const long long *mom, double v, wc_map_surfel *out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = skeys[i];
  const uint64_t slot = sslots[i];
  const long long *p = pay + 4 * slot;
  const double c = (double)p[3];
  const map_plane pl = map_plane_of(p[3], mom + kMapMom * slot);
  wc_map_surfel r;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int k = map_unpack(key, a);
    r.key[a] = k;
    r.xyz[a] = map_centroid(k, v, p[a], c);
    r.ev[a] = pl.ev[a];
    r.normal[a] = pl.nrm[a];
  }
  r.count = (uint32_t)p[3];
  r.flags = pl.plane;
#pragma unroll
  for (int e = 0; e < 6; ++e) r.cov[e] = pl.cov[e];
  out[i] = r;
}

// query: the nearest of the occupied voxels with index kq + {-1, 0, 1}^3 (kq = the query's own voxel), by the fp64 distance to the float
// centroid wc_map_export returns.  One lane per query.  The 27 neighbours are visited in ascending key order (x outermost) and a later
// one wins only on a strictly smaller distance: ties go to the smaller key.  Each x plane's nine first-slot key loads are issued together
// before any is looked at; a lane then follows the probe chain (read-only) of whatever is not settled by its first slot, and loads the
// 32-byte payload of the occupied ones only.  Every loop below is fully unrolled: all indices are compile-time constants, no scratch.
// PLANE (wc_map_nearest_plane): the record is a wc_map_plane_hit - the same 40 bytes, then the winning voxel's plane from map_plane_of,
// run once per query behind the search - and `hits` points at those records; mom and min_points are unused otherwise
// what the search says about one query: the winner's centroid, count, index, slot and squared distance
struct map_found {
  double best;
  float bx, by, bz;
  unsigned bc;
  int bkx, bky, bkz;
  unsigned long long bh;  // (PLANE: the winner's slot)
  bool ok;                // the query could be searched
};
// the search of one query (x, y, z) - the body k_map_nearest and k_map_linearize share
template <bool PLANE>
__device__ __forceinline__ map_found map_search(double x, double y, double z, double v, const unsigned long long *keys, const long long *pay,
                                                unsigned long long mask) {
  int kx, ky, kz;
  const bool ok = map_voxel_of(x, y, z, v, kx, ky, kz);  // (an unsearchable query: voxel 0, found nothing - see `in`)
  double best = __builtin_inf();
  float bx = 0.f, by = 0.f, bz = 0.f;
  unsigned bc = 0;
  int bkx = 0, bky = 0, bkz = 0;
  unsigned long long bh = 0;
#pragma unroll
  for (int dx = -1; dx <= 1; ++dx) {
    unsigned long long key[9], h[9], cur[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int nx = kx + dx, ny = ky + (j / 3 - 1), nz = kz + (j % 3 - 1);
      // (a neighbour beyond the key range holds nothing: its "key" is the empty mark, which the first slot read then settles)
      const bool in = ok && nx > -kMapKeyOff && nx < kMapKeyOff && ny > -kMapKeyOff && ny < kMapKeyOff && nz > -kMapKeyOff && nz < kMapKeyOff;
      key[j] = in ? map_pack(nx, ny, nz) : kMapEmpty;
      h[j] = in ? map_hash(key[j]) & mask : 0;
      cur[j] = keys[h[j]];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      if (key[j] == kMapEmpty) continue;
      unsigned long long hj = h[j];
      if (!map_find_from(keys, mask, key[j], hj, cur[j])) continue;
      const longlong2 *p = (const longlong2 *)(pay + 4 * hj);
      const longlong2 p0 = p[0], p1 = p[1];
      const double cnt = (double)p1.y;
      const int nx = kx + dx, ny = ky + (j / 3 - 1), nz = kz + (j % 3 - 1);
      const float cx = map_centroid(nx, v, p0.x, cnt), cy = map_centroid(ny, v, p0.y, cnt), cz = map_centroid(nz, v, p1.x, cnt);
      const double ex = x - (double)cx, ey = y - (double)cy, ez = z - (double)cz;
      const double d2 = (ex * ex + ey * ey) + ez * ez;
      if (d2 < best) {
        best = d2, bx = cx, by = cy, bz = cz, bc = (unsigned)p1.y, bkx = nx, bky = ny, bkz = nz;
        if constexpr (PLANE) bh = hj;
      }
    }
  }
  return map_found{best, bx, by, bz, bc, bkx, bky, bkz, bh, ok};
}
// the plane of an accepted winner (hit: bc != 0 and best <= max_d2): normal, sigma2 and the signed distance of the query; false (and
// all of them 0) unless the voxel holds min_points points and its plane bit is set - flags bit 1 of a wc_map_plane_hit
__device__ __forceinline__ bool map_hit_plane(const map_found &w, bool hit, double x, double y, double z, const long long *mom, unsigned min_points,
                                              double (&pn)[3], double &sigma2, double &dist) {
  bool valid = false;
  pn[0] = 0.0, pn[1] = 0.0, pn[2] = 0.0, sigma2 = 0.0, dist = 0.0;
  if (hit && w.bc >= min_points) {
    const map_plane pl = map_plane_of((long long)w.bc, mom + kMapMom * w.bh);
    if (pl.plane) {
      const double ex = x - (double)w.bx, ey = y - (double)w.by, ez = z - (double)w.bz;  // (as in d2)
      pn[0] = pl.nrm[0], pn[1] = pl.nrm[1], pn[2] = pl.nrm[2], sigma2 = pl.ev[0];
      dist = (pn[0] * ex + pn[1] * ey) + pn[2] * ez;
      valid = true;
    }
  }
  return valid;
}

template <bool PLANE>
__global__ void __launch_bounds__(kNearThreads) k_map_nearest(wc_points q, double v, double max_d2, const unsigned long long *keys,
                                                              const long long *pay, unsigned long long mask, void *hits,
                                                              unsigned long long *found, const long long *mom, unsigned min_points) {
  unsigned n_found = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kNearThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kNearThreads + threadIdx.x; i < q.n; i += stride) {
    const float *f = (const float *)((const char *)q.xyz + i * q.xyz_stride);
    const double x = (double)f[0], y = (double)f[1], z = (double)f[2];
    const map_found w = map_search<PLANE>(x, y, z, v, keys, pay, mask);
    const bool hit = w.bc != 0 && w.best <= max_d2;
    n_found += hit ? 1u : 0u;
    // the 40-byte record as five 8-byte stores (the record is 8-aligned)
    uint2 *o = (uint2 *)((char *)hits + i * (PLANE ? sizeof(wc_map_plane_hit) : sizeof(wc_map_hit)));
    unsigned flags = w.ok ? 0u : 1u;
    if constexpr (PLANE) {
      double pn[3], sigma2, dist;
      flags |= map_hit_plane(w, hit, x, y, z, mom, min_points, pn, sigma2, dist) ? 2u : 0u;
      double *od = (double *)o;
      od[5] = pn[0], od[6] = pn[1], od[7] = pn[2], od[8] = sigma2, od[9] = dist;
    }
    o[0] = hit ? make_uint2(__float_as_uint(w.bx), __float_as_uint(w.by)) : make_uint2(0u, 0u);
    o[1] = hit ? make_uint2(__float_as_uint(w.bz), w.bc) : make_uint2(0u, 0u);
    o[2] = hit ? make_uint2((unsigned)w.bkx, (unsigned)w.bky) : make_uint2(0u, 0u);
    o[3] = make_uint2(hit ? (unsigned)w.bkz : 0u, flags);
    ((double *)o)[4] = hit ? w.best : __builtin_inf();
  }
  block_count<kNearThreads>({n_found}, {found});
}

// k nearest within a radius (wc_map_knn): the candidates are the occupied voxels of kq + {-REACH .. REACH}^3 that hold min_points points
// (and, with not_own, are not kq itself), the distance is map_search's d2, a candidate is accepted iff d2 <= max_d2, and the answer is
// the accepted ones in ascending (d2, key).  One lane per query, grid-strided.  The neighbours are visited in ascending key order (x
// outermost), a batch at a time - an x plane of nine (REACH 1) or a z row of five (REACH 2) - whose first-slot key loads are issued
// before any is looked at, as map_search does; the batches are a rolled loop, so the code is one batch long.  The list is KMAX entries
// of (d2, slot) in registers, kept sorted by a fully unrolled compare-and-shift (every index a compile-time constant: no scratch) that
// moves a candidate in front of an entry only on a strictly smaller d2: ties keep the visiting order, the key order, with no key
// compare.  An entry's centroid, count and index are formed again from its slot at write-out, by the expressions the search used.
constexpr int kKnnThreads = 256;
template <int KMAX>
struct map_knn_list {
  double d[KMAX];
  unsigned s[KMAX];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) d[j] = __builtin_inf(), s[j] = 0u;
  }
  // entry j becomes the candidate, its predecessor or itself; descending j reads only entries not yet rewritten
  __device__ __forceinline__ void insert(double d2, unsigned slot) {
#pragma unroll
    for (int j = KMAX - 1; j >= 0; --j) {
      const bool here = d2 < d[j];
      bool up = false;
      if constexpr (KMAX > 1)
        if (j > 0) up = d2 < d[j > 0 ? j - 1 : 0];
      const double pd = up ? d[j > 0 ? j - 1 : 0] : d2;
      const unsigned ps = up ? s[j > 0 ? j - 1 : 0] : slot;
      d[j] = here ? pd : d[j];
      s[j] = here ? ps : s[j];
    }
  }
};

template <int KMAX, int REACH>
__global__ void __launch_bounds__(kKnnThreads) k_map_knn(wc_points q, double v, double max_d2, unsigned k, unsigned min_points, unsigned not_own,
                                                         const unsigned long long *keys, const long long *pay, unsigned long long mask,
                                                         wc_map_hit *hits, uint32_t *within, unsigned long long *n_some,
                                                         unsigned long long *n_rec, unsigned long long *n_within) {
  constexpr int W = 2 * REACH + 1;
  constexpr int B = REACH == 1 ? 9 : 5;  // neighbours of a batch
  constexpr int NB = W * W * W / B;      // 3 planes, 25 rows
  unsigned long long c_some = 0, c_rec = 0, c_within = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kKnnThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kKnnThreads + threadIdx.x; i < q.n; i += stride) {
    const float *f = (const float *)((const char *)q.xyz + i * q.xyz_stride);
    const double x = (double)f[0], y = (double)f[1], z = (double)f[2];
    int kx, ky, kz;
    const bool ok = map_voxel_of(x, y, z, v, kx, ky, kz);
    map_knn_list<KMAX> L;
    L.clear();
    unsigned nw = 0;
    if (ok) {
#pragma unroll 1
      for (int b = 0; b < NB; ++b) {
        const int bx = REACH == 1 ? b - 1 : b / W - REACH, by = REACH == 1 ? 0 : b % W - REACH;  // (REACH 1: y and z come from j)
        unsigned long long key[B], h[B], cur[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
          const int ox = bx, oy = REACH == 1 ? j / 3 - 1 : by, oz = REACH == 1 ? j % 3 - 1 : j - REACH;
          const int nx = kx + ox, ny = ky + oy, nz = kz + oz;
          // (a neighbour beyond the key range, or the query's own voxel under not_own: the empty mark, as in map_search)
          const bool in = nx > -kMapKeyOff && nx < kMapKeyOff && ny > -kMapKeyOff && ny < kMapKeyOff && nz > -kMapKeyOff && nz < kMapKeyOff &&
                          !(not_own && (ox | oy | oz) == 0);
          key[j] = in ? map_pack(nx, ny, nz) : kMapEmpty;
          h[j] = in ? map_hash(key[j]) & mask : 0;
          cur[j] = keys[h[j]];
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
          if (key[j] == kMapEmpty) continue;
          unsigned long long hj = h[j];
          if (!map_find_from(keys, mask, key[j], hj, cur[j])) continue;
          const longlong2 *p = (const longlong2 *)(pay + 4 * hj);
          const longlong2 p0 = p[0], p1 = p[1];
          if ((unsigned long long)p1.y < min_points) continue;
          const double cnt = (double)p1.y;
          const int nx = kx + bx, ny = ky + (REACH == 1 ? j / 3 - 1 : by), nz = kz + (REACH == 1 ? j % 3 - 1 : j - REACH);
          const float cx = map_centroid(nx, v, p0.x, cnt), cy = map_centroid(ny, v, p0.y, cnt), cz = map_centroid(nz, v, p1.x, cnt);
          const double ex = x - (double)cx, ey = y - (double)cy, ez = z - (double)cz;
          const double d2 = (ex * ex + ey * ey) + ez * ez;
          if (!(d2 <= max_d2)) continue;
          ++nw;
          if (d2 < L.d[KMAX - 1]) L.insert(d2, (unsigned)hj);
        }
      }
    }
    const unsigned n_out = nw < k ? nw : k;
    c_some += nw ? 1u : 0u, c_rec += n_out, c_within += nw;
    if (within) within[i] = nw;
    // the k 40-byte records as five 8-byte stores each (the records are 8-aligned)
    uint2 *o = (uint2 *)(hits + i * k);
    const unsigned flags = ok ? 0u : 1u;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if ((unsigned)j >= k) continue;  // (k <= KMAX)
      if ((unsigned)j < n_out) {
        const unsigned long long hj = L.s[j], key = keys[hj];
        const longlong2 *p = (const longlong2 *)(pay + 4 * hj);
        const longlong2 p0 = p[0], p1 = p[1];
        const double cnt = (double)p1.y;
        const int nx = map_unpack(key, 0), ny = map_unpack(key, 1), nz = map_unpack(key, 2);
        const float cx = map_centroid(nx, v, p0.x, cnt), cy = map_centroid(ny, v, p0.y, cnt), cz = map_centroid(nz, v, p1.x, cnt);
        o[5 * j + 0] = make_uint2(__float_as_uint(cx), __float_as_uint(cy));
        o[5 * j + 1] = make_uint2(__float_as_uint(cz), (unsigned)p1.y);
        o[5 * j + 2] = make_uint2((unsigned)nx, (unsigned)ny);
        o[5 * j + 3] = make_uint2((unsigned)nz, flags);
        ((double *)o)[5 * j + 4] = L.d[j];
      } else {
        o[5 * j + 0] = make_uint2(0u, 0u), o[5 * j + 1] = make_uint2(0u, 0u), o[5 * j + 2] = make_uint2(0u, 0u);
        o[5 * j + 3] = make_uint2(0u, flags);
        ((double *)o)[5 * j + 4] = __builtin_inf();
      }
    }
  }
  block_count<kKnnThreads>({c_some, c_rec, c_within}, {n_some, n_rec, n_within});
}

// ---- registration (wc_map_linearize) ----------------------------------------------------------------------------------------------
// The plane query with another ending: the point goes through the pose first, and instead of an 80-byte record its 8-double row
// (J, d, k) and its rho enter the sums of the point-to-plane normal equations.  Summation order (a function of the point count alone):
//   tile t = points [256 t, 256 t + 256): every lane leaves row and rho in LDS (unused points and the points past n: zeros); lane
//   (e, c), e < 28 sums, c < 8 chunks, adds the terms of rows 32 c .. 32 c + 31 in ascending order (31 additions), lane e < 28 then adds
//   the eight chunk sums in ascending order (7 additions): 38 additions per term, whichever workgroup works on the tile.  One
//   256-byte partial per tile: 28 doubles, then the integer counts n_used, n_found, n_bad (finite points the pose sent to a non-finite
//   one) and a zero word, written with plain vector stores.
//   k_map_lin_reduce: partial j of level l + 1 = partials 32 j .. 32 j + 31 of level l added in ascending order, one launch per level
//   (of every hypothesis) until one partial is left (the launch boundary is the hand-off: no ticket, no fence, no atomics on doubles).
constexpr int kLinThreads = 256;
constexpr int kLinSums = 28;    // H's upper triangle (21), g (6), sum rho (1)
constexpr int kLinWords = 32;   // 8-byte words of a partial
constexpr int kLinFan = 32;     // partials (and rows) added sequentially into one
constexpr int kLinFields = 9;   // J[6], d, k, rho
constexpr int kLinPitch = kLinThreads + kLinThreads / kLinFan;  // rows of one field in LDS: one word of padding per chunk of 32
struct map_pose {
  double T[12];
};
struct map_reg {
  double max_d2, s02, a2;  // max_dist^2, sigma0^2, cauchy_a^2 (0: no loss): each product formed once on the host
  unsigned min_points;
};

// a point through a pose: q_a = (float)(((T[4a] x + T[4a+1] y) + T[4a+2] z) + T[4a+3]) with x, y, z the floats cast to double - the
// registration's and the score's one copy (include/wildcat_hip.h states the association; -ffp-contract=off: no fused multiply-add)
__device__ __forceinline__ void map_move(const double (&T)[12], float px, float py, float pz, float &qx, float &qy, float &qz) {
  const double x0 = (double)px, y0 = (double)py, z0 = (double)pz;
  qx = (float)(((T[0] * x0 + T[1] * y0) + T[2] * z0) + T[3]);
  qy = (float)(((T[4] * x0 + T[5] * y0) + T[6] * z0) + T[7]);
  qz = (float)(((T[8] * x0 + T[9] * y0) + T[10] * z0) + T[11]);
}

// one tile of k_map_linearize.  T: the pose (workgroup uniform); out: the tile's 256-byte partial;
// rows: NULL or the call's wc_map_reg_row array; s_row, s_chunk, s_cnt: the workgroup's LDS (kLinFields * kLinPitch and kLinSums * 8
// doubles, 3 words).  Every lane of the workgroup calls it
__device__ __forceinline__ void map_lin_tile(const wc_points &pts, const double (&T)[12], const map_reg &R, double v, const unsigned long long *keys,
                                             const long long *pay, const long long *mom, unsigned long long mask, wc_map_reg_row *rows,
                                             uint64_t tile, unsigned long long *out, double *s_row, double *s_chunk, unsigned *s_cnt) {
  const int t = threadIdx.x;
  if (t < 3) s_cnt[t] = 0;
  __syncthreads();  // (also: the previous tile's sums have been read)
  const uint64_t i = tile * kLinThreads + t;
  double row[kLinFields] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool used = false, hit = false, bad = false;
  if (i < pts.n) {
    const float *f = (const float *)((const char *)pts.xyz + i * pts.xyz_stride);
    const float px = f[0], py = f[1], pz = f[2];
    float qx, qy, qz;
    map_move(T, px, py, pz, qx, qy, qz);
    bad = isfinite(px) && isfinite(py) && isfinite(pz) && !(isfinite(qx) && isfinite(qy) && isfinite(qz));
    const double x = (double)qx, y = (double)qy, z = (double)qz;
    const map_found w = map_search<true>(x, y, z, v, keys, pay, mask);
    hit = w.bc != 0 && w.best <= R.max_d2;
    double pn[3], sigma2, dist;
    used = map_hit_plane(w, hit, x, y, z, mom, R.min_points, pn, sigma2, dist);
    if (used) {
      row[0] = y * pn[2] - z * pn[1], row[1] = z * pn[0] - x * pn[2], row[2] = x * pn[1] - y * pn[0];
      row[3] = pn[0], row[4] = pn[1], row[5] = pn[2];
      row[6] = dist;
      const double w2 = 1.0 / (R.s02 + sigma2), s = (w2 * dist) * dist;
      if (R.a2 > 0.0) {
        const double u = s / R.a2;
        row[7] = w2 / (1.0 + u), row[8] = R.a2 * log1p(u);
      } else {
        row[7] = w2, row[8] = s;
      }
    }
    if (rows) {  // (the record is 8-aligned: eight 8-byte stores)
      double *o = (double *)(rows + i);
#pragma unroll
      for (int fld = 0; fld < 8; ++fld) o[fld] = row[fld];
    }
  }
  // the counts: per wavefront, then integer adds in LDS (order independent)
  const unsigned n_u = (unsigned)__popcll(__ballot(used)), n_h = (unsigned)__popcll(__ballot(hit)), n_b = (unsigned)__popcll(__ballot(bad));
  if ((t & 63) == 0) {
    if (n_u) atomicAdd(&s_cnt[0], n_u);
    if (n_h) atomicAdd(&s_cnt[1], n_h);
    if (n_b) atomicAdd(&s_cnt[2], n_b);
  }
  const int at = t + t / kLinFan;
#pragma unroll
  for (int fld = 0; fld < kLinFields; ++fld) s_row[fld * kLinPitch + at] = row[fld];
  __syncthreads();
  if (t < kLinSums * 8) {
    const int e = t >> 3, c = t & 7;
    // e -> the three factors of a term (k X) Y: H(a, b): X = J_a, Y = J_b; g_a: X = J_a, Y = d; sum rho: the term itself
    int a = 0, b = e;
    while (b >= 6 - a && a < 6) b -= 6 - a, ++a;
    const int fx = e < 21 ? a : e - 21, fy = e < 21 ? a + b : 6;
    const double *rk = s_row + 7 * kLinPitch + c * (kLinFan + 1), *rx = s_row + fx * kLinPitch + c * (kLinFan + 1),
                 *ry = s_row + fy * kLinPitch + c * (kLinFan + 1), *rr = s_row + 8 * kLinPitch + c * (kLinFan + 1);
    double acc = 0.0;
    if (e < 27) {
      acc = (rk[0] * rx[0]) * ry[0];
      for (int j = 1; j < kLinFan; ++j) acc += (rk[j] * rx[j]) * ry[j];
    } else {
      acc = rr[0];
      for (int j = 1; j < kLinFan; ++j) acc += rr[j];
    }
    s_chunk[e * 8 + c] = acc;
  }
  __syncthreads();
  if (t < kLinWords) {
    unsigned long long word = 0;
    if (t < kLinSums) {
      double acc = s_chunk[t * 8];
#pragma unroll
      for (int c = 1; c < 8; ++c) acc += s_chunk[t * 8 + c];
      word = (unsigned long long)__double_as_longlong(acc);
    } else if (t < kLinSums + 3) {
      word = s_cnt[t - kLinSums];
    }
    out[t] = word;
  }
}

// The registration's first kernel in its two forms, one body.  ONE: one pose, carried in the kernel arguments (P; poses and K
// are not read), the work items are the tiles and rows may be non-null.  Otherwise K poses in a device array (poses: K x 12 doubles, read
// through loads whose address is the same for the whole workgroup; P and rows are not read), and a work item is a (hypothesis, tile)
// pair, item = h * tiles + tile: neighbouring workgroups share a hypothesis and work on neighbouring tiles of it.  Items are counted in
// 64 bits in both forms: no cap on n comes from here.  part: hypothesis-major, hyp_words words each
template <bool ONE>
__global__ void __launch_bounds__(kLinThreads) k_map_linearize(wc_points pts, map_pose P, const double *__restrict__ poses, unsigned K, map_reg R,
                                                               double v, const unsigned long long *keys, const long long *pay,
                                                               const long long *mom, unsigned long long mask, wc_map_reg_row *rows,
                                                               unsigned long long *part, unsigned long long hyp_words) {
  __shared__ double s_row[kLinFields * kLinPitch];
  __shared__ double s_chunk[kLinSums * 8];
  __shared__ unsigned s_cnt[3];
  const uint64_t tiles = (pts.n + kLinThreads - 1) / kLinThreads, items = ONE ? tiles : (uint64_t)K * tiles;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t h = ONE ? 0 : item / tiles, tile = item - h * tiles;
    const double *Tp = ONE ? P.T : poses + h * 12;
    double T[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) T[j] = Tp[j];
    map_lin_tile(pts, T, R, v, keys, pay, mom, mask, ONE ? rows : nullptr, tile, part + h * hyp_words + tile * kLinWords, s_row, s_chunk, s_cnt);
  }
}

// ---- occupancy score of pose hypotheses (wc_map_score_batch: DESIGN 8.11) -----------------------------------------------------------
// A workgroup keeps ONE tile of 256 points in registers, one point per lane, and walks a block of kScoreBlock hypotheses with it.  A work
// item is a (hypothesis block, tile) pair, item = block * tiles + tile: neighbouring workgroups share the poses and read neighbouring
// tiles.  The pose of a hypothesis is read at an address the whole workgroup shares (scalar loads).  BATCH hypotheses go together: their
// moved points, keys, hashes and first-slot key loads first, then the chains and the count loads.  The three counts of a hypothesis: ballot
// and popcount per wavefront, integer adds in LDS across the four wavefronts, then one 32-bit atomic add per workgroup, hypothesis and
// non-zero count into out (K x 4 words, zeroed ahead of the launch).  Integer adds commute: the records do not depend on the grid, the
// schedule or the run, and the launch boundary is the hand-off.
constexpr int kScoreThreads = 256;
constexpr int kScoreBlock = 32;  // hypotheses one work item walks with its tile
constexpr int kScoreBatch = 8;   // hypotheses whose first-slot key loads are in flight together (as kCarveBatch, kCastBatch)
template <int BATCH>
__global__ void __launch_bounds__(kScoreThreads) k_map_score_batch(wc_points pts, const double *__restrict__ poses, unsigned K, double v,
                                                                   const unsigned long long *__restrict__ keys, const long long *__restrict__ pay,
                                                                   unsigned long long mask, unsigned min_points, unsigned *out) {
  static_assert(kScoreBlock % BATCH == 0, "a block is a whole number of batches");
  __shared__ unsigned s_cnt[kScoreBlock * 3];
  const int t = threadIdx.x;
  const unsigned long long tiles = (pts.n + kScoreThreads - 1) / kScoreThreads;
  const unsigned long long items = (unsigned long long)((K + kScoreBlock - 1) / kScoreBlock) * tiles;  // (<= 2^15 * 2^23)
  if (t < kScoreBlock * 3) s_cnt[t] = 0;
  for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {
    const unsigned long long blk = item / tiles, tile = item - blk * tiles;
    const unsigned h_first = (unsigned)blk * kScoreBlock;
    const unsigned h_count = K - h_first < (unsigned)kScoreBlock ? K - h_first : (unsigned)kScoreBlock;
    __syncthreads();  // (the zeros of s_cnt are in place: the first ones, or those the previous item's readers left)
    const unsigned long long i = tile * kScoreThreads + t;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    bool valid = false;
    if (i < pts.n) {
      const float *f = (const float *)((const char *)pts.xyz + i * pts.xyz_stride);
      px = f[0], py = f[1], pz = f[2];
      valid = isfinite(px) && isfinite(py) && isfinite(pz);
    }
    for (unsigned b = 0; b < h_count; b += BATCH) {
      unsigned long long key[BATCH], slot[BATCH], first[BATCH];
      bool in[BATCH], bad[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        in[j] = bad[j] = false;
        key[j] = slot[j] = 0, first[j] = kMapEmpty;
        if (b + j < h_count) {  // (workgroup uniform)
          const double *Tp = poses + (size_t)(h_first + b + j) * 12;
          double T[12];
#pragma unroll
          for (int e = 0; e < 12; ++e) T[e] = Tp[e];
          float qx, qy, qz;
          map_move(T, px, py, pz, qx, qy, qz);
          const bool fin = isfinite(qx) && isfinite(qy) && isfinite(qz);
          int kx, ky, kz;
          const bool ok = map_voxel_of((double)qx, (double)qy, (double)qz, v, kx, ky, kz);  // (false for a non-finite q: the compares fail)
          bad[j] = valid && !fin;
          in[j] = valid && fin && ok;
          key[j] = map_pack(kx, ky, kz);
          slot[j] = map_hash(key[j]) & mask;  // (always inside the table: the load below needs no further bound)
          if (in[j]) first[j] = keys[slot[j]];
        }
      }
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        if (b + j < h_count) {
          bool hit = false;
          if (in[j] && map_find_from(keys, mask, key[j], slot[j], first[j])) hit = (unsigned long long)pay[4 * slot[j] + 3] >= min_points;
          const unsigned n_h = (unsigned)__popcll(__ballot(hit)), n_i = (unsigned)__popcll(__ballot(in[j])),
                         n_b = (unsigned)__popcll(__ballot(bad[j]));
          if ((t & 63) == 0) {
            if (n_h) atomicAdd(&s_cnt[(b + j) * 3 + 0], n_h);
            if (n_i) atomicAdd(&s_cnt[(b + j) * 3 + 1], n_i);
            if (n_b) atomicAdd(&s_cnt[(b + j) * 3 + 2], n_b);
          }
        }
      }
    }
    __syncthreads();
    if (t < kScoreBlock * 3) {
      const unsigned c = s_cnt[t], hl = (unsigned)t / 3;
      s_cnt[t] = 0;
      if (c && hl < h_count) atomicAdd(out + (size_t)(h_first + hl) * 4 + ((unsigned)t - 3 * hl), c);
    }
  }
}

// word e of partial j of the next level: in[32 j] + in[32 j + 1] + ... in ascending order (the doubles; the counts are integers); m: the
// partials of `in`, 32 j < m.  WORDS: the 8-byte words of a partial, the first SUMS of them doubles (32 and 28: the rigid registration's;
// 80 and 76: the continuous-time one's)
template <int WORDS, int SUMS>
__device__ __forceinline__ void map_lin_reduce_word(const unsigned long long *in, uint64_t m, uint64_t j, int e, unsigned long long *out) {
  const uint64_t first = j * kLinFan;
  const uint64_t cnt = m - first < (uint64_t)kLinFan ? m - first : (uint64_t)kLinFan;
  const unsigned long long *p = in + first * WORDS + e;
  unsigned long long word = p[0];
  if (e < SUMS) {
    double acc = __longlong_as_double((long long)word);
    for (uint64_t r = 1; r < cnt; ++r) acc += __longlong_as_double((long long)p[r * WORDS]);
    word = (unsigned long long)__double_as_longlong(acc);
  } else {
    for (uint64_t r = 1; r < cnt; ++r) word += p[r * WORDS];
  }
  out[j * WORDS + e] = word;
}

// one level of the second stage for all K hypotheses, one lane per word of the next level: hypothesis h reads its m partials at
// in + h * in_stride and writes its ceil(m / 32) at out + h * out_stride (words)
template <int WORDS, int SUMS>
__global__ void __launch_bounds__(256) k_map_lin_reduce(const unsigned long long *in, uint64_t in_stride, uint64_t m, unsigned long long *out,
                                                        uint64_t out_stride, unsigned K) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t per = (m + kLinFan - 1) / kLinFan * WORDS;  // words of one hypothesis's next level
  if (g >= K * per) return;
  const uint64_t h = K == 1 ? 0 : g / per, r = g - h * per;  // (one pose: no division by a run-time value, as before the K-pose form)
  map_lin_reduce_word<WORDS, SUMS>(in + h * in_stride, m, r / WORDS, (int)(r % WORDS), out + h * out_stride);
}

// ---- registration of a stamped sweep in continuous time (wc_map_linearize_ct: DESIGN 8.12) -------------------------------------------
// k_map_linearize<true> with the point's own pose: interpolated between a begin and an end pose by the point's stamp (map_move_ct: the
// normalised linear blend, include/wildcat_hip.h states the associations), and a row that carries the two poses' shares a = 1 - s and s.
// 76 sums - H00, H01, H11 (21 each), g0, g1 (6 each), sum rho - in k_map_linearize's order: lane (e, c) adds the terms of rows
// 32 c .. 32 c + 31 in ascending order, 76 x 8 pairs over 256 lanes in three rounds, then lane e adds the eight chunk sums in ascending
// order.  One 640-byte partial per tile: 76 doubles, then n_used, n_found, n_outside, n_bad, written with plain vector stores; the
// levels are k_map_lin_reduce<80, 76>.
constexpr int kCtSums = 76;
constexpr int kCtWords = 80;
constexpr int kCtFields = 13;  // J[6], d, rho, kaa, kab, kbb, ka, kb
struct map_ct_pose {
  double p0[3], q0[4], p1[3], q1[4];  // pos and quat (w, x, y, z) of the begin and of the end pose; q1 on q0's side (the host negates it)
  double t_begin, t_end, span;
};
// the stamp test and the share of the end pose: false (and s = 0) for a stamp outside [t_begin, t_end] or NaN
__host__ __device__ inline bool map_ct_share(const map_ct_pose &C, double t, double &s) {
  const bool in = t >= C.t_begin && t <= C.t_end;
  s = in ? (t - C.t_begin) / C.span : 0.0;
  return in;
}
// a point through the pose interpolated at s - the device's and wc_pose_interp_move's one copy (-ffp-contract=off: no fused multiply-add)
__host__ __device__ inline void map_move_ct(const map_ct_pose &C, double s, float fx, float fy, float fz, float &ox, float &oy, float &oz) {
  const double a = 1.0 - s, px = (double)fx, py = (double)fy, pz = (double)fz;
  const double qw = a * C.q0[0] + s * C.q1[0], qx = a * C.q0[1] + s * C.q1[1], qy = a * C.q0[2] + s * C.q1[2], qz = a * C.q0[3] + s * C.q1[3];
  const double cx = a * C.p0[0] + s * C.p1[0], cy = a * C.p0[1] + s * C.p1[1], cz = a * C.p0[2] + s * C.p1[2];
  const double nn = ((qw * qw + qx * qx) + qy * qy) + qz * qz, f = 2.0 / nn;
  const double ux = qy * pz - qz * py, uy = qz * px - qx * pz, uz = qx * py - qy * px;
  const double rx = qy * uz - qz * uy, ry = qz * ux - qx * uz, rz = qx * uy - qy * ux;
  ox = (float)((px + f * (qw * ux + rx)) + cx);
  oy = (float)((py + f * (qw * uy + ry)) + cy);
  oz = (float)((pz + f * (qw * uz + rz)) + cz);
}

__global__ void __launch_bounds__(kLinThreads) k_map_linearize_ct(wc_points pts, map_ct_pose C, map_reg R, double v, const unsigned long long *keys,
                                                                  const long long *pay, const long long *mom, unsigned long long mask,
                                                                  wc_map_ct_row *rows, float *xyz_out, unsigned long long *part) {
  __shared__ double s_row[kCtFields * kLinPitch];
  __shared__ double s_chunk[kCtSums * 8];
  __shared__ unsigned s_cnt[4];
  const int t = threadIdx.x;
  const uint64_t tiles = (pts.n + kLinThreads - 1) / kLinThreads;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // lanes 0 .. 3 own the count words: they zero them here and are the only lanes that read them, at the tile's end (below) - the same
    // lane reads, then zeroes, in program order, so no barrier is needed between one tile's read and the next tile's zero
    if (t < 4) s_cnt[t] = 0;
    __syncthreads();  // (also: the previous tile's rows and chunk sums have been read - their next writes lie behind this barrier)
    const uint64_t i = tile * kLinThreads + t;
    double row[kCtFields] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool used = false, hit = false, bad = false, outside = false;
    if (i < pts.n) {
      const float *f = (const float *)((const char *)pts.xyz + i * pts.xyz_stride);
      const float px = f[0], py = f[1], pz = f[2];
      const double stamp = *(const double *)((const char *)pts.time + i * pts.time_stride);
      double s;
      const bool in = map_ct_share(C, stamp, s);
      outside = !in;
      float qx = __uint_as_float(0x7fc00000u), qy = qx, qz = qx;
      double k = 0.0;
      if (in) {
        map_move_ct(C, s, px, py, pz, qx, qy, qz);
        bad = isfinite(px) && isfinite(py) && isfinite(pz) && !(isfinite(qx) && isfinite(qy) && isfinite(qz));
        const double x = (double)qx, y = (double)qy, z = (double)qz;
        const map_found w = map_search<true>(x, y, z, v, keys, pay, mask);
        hit = w.bc != 0 && w.best <= R.max_d2;
        double pn[3], sigma2, dist;
        used = map_hit_plane(w, hit, x, y, z, mom, R.min_points, pn, sigma2, dist);
        if (used) {
          row[0] = y * pn[2] - z * pn[1], row[1] = z * pn[0] - x * pn[2], row[2] = x * pn[1] - y * pn[0];
          row[3] = pn[0], row[4] = pn[1], row[5] = pn[2];
          row[6] = dist;
          const double w2 = 1.0 / (R.s02 + sigma2), s2 = (w2 * dist) * dist;
          if (R.a2 > 0.0) {
            const double u = s2 / R.a2;
            k = w2 / (1.0 + u), row[7] = R.a2 * log1p(u);
          } else {
            k = w2, row[7] = s2;
          }
          const double a = 1.0 - s, ka = k * a, kb = k * s;
          row[8] = ka * a, row[9] = ka * s, row[10] = kb * s, row[11] = ka, row[12] = kb;
        }
      }
      if (rows) {  // (the record is 8-aligned: nine 8-byte stores)
        double *o = (double *)(rows + i);
#pragma unroll
        for (int fld = 0; fld < 7; ++fld) o[fld] = row[fld];
        o[7] = k, o[8] = used ? s : 0.0;
      }
      if (xyz_out) xyz_out[3 * i] = qx, xyz_out[3 * i + 1] = qy, xyz_out[3 * i + 2] = qz;
    }
    // the counts: per wavefront, then integer adds in LDS (order independent)
    const unsigned n_u = (unsigned)__popcll(__ballot(used)), n_h = (unsigned)__popcll(__ballot(hit)), n_o = (unsigned)__popcll(__ballot(outside)),
                   n_b = (unsigned)__popcll(__ballot(bad));
    if ((t & 63) == 0) {
      if (n_u) atomicAdd(&s_cnt[0], n_u);
      if (n_h) atomicAdd(&s_cnt[1], n_h);
      if (n_o) atomicAdd(&s_cnt[2], n_o);
      if (n_b) atomicAdd(&s_cnt[3], n_b);
    }
    const int at = t + t / kLinFan;
#pragma unroll
    for (int fld = 0; fld < kCtFields; ++fld) s_row[fld * kLinPitch + at] = row[fld];
    __syncthreads();
#pragma unroll
    for (int round = 0; round < (kCtSums * 8 + kLinThreads - 1) / kLinThreads; ++round) {
      const int pair = round * kLinThreads + t;
      if (pair < kCtSums * 8) {
        const int e = pair >> 3, c = pair & 7;
        // e -> the three factors of a term (W X) Y: a block of H: W = kaa, kab or kbb, X = J_a, Y = J_b; g0, g1: W = ka or kb, X = J_a, Y = d
        int fw, fx, fy = 6;
        if (e < 63) {  // entry idx of block blk -> (a, a + b) of the upper triangle
          const int blk = e / 21, idx = e - 21 * blk;
          int a = 0, b = idx;
          while (b >= 6 - a) b -= 6 - a, ++a;
          fw = 8 + blk, fx = a, fy = a + b;
        } else if (e < 69) {
          fw = 11, fx = e - 63;
        } else {
          fw = 12, fx = e < 75 ? e - 69 : 0;  // (e = 75: sum rho, no factors)
        }
        const int at_c = c * (kLinFan + 1);
        double acc;
        if (e < 75) {
          const double *rw = s_row + fw * kLinPitch + at_c, *rx = s_row + fx * kLinPitch + at_c, *ry = s_row + fy * kLinPitch + at_c;
          acc = (rw[0] * rx[0]) * ry[0];
          for (int j = 1; j < kLinFan; ++j) acc += (rw[j] * rx[j]) * ry[j];
        } else {
          const double *rr = s_row + 7 * kLinPitch + at_c;
          acc = rr[0];
          for (int j = 1; j < kLinFan; ++j) acc += rr[j];
        }
        s_chunk[e * 8 + c] = acc;
      }
    }
    __syncthreads();
    if (t < kCtSums) {
      double acc = s_chunk[t * 8];
#pragma unroll
      for (int c = 1; c < 8; ++c) acc += s_chunk[t * 8 + c];
      part[tile * kCtWords + t] = (unsigned long long)__double_as_longlong(acc);
    }
    if (t < kCtWords - kCtSums) part[tile * kCtWords + kCtSums + t] = s_cnt[t];  // (the lanes that zero them for the next tile)
  }
}

// the occupied slots that `sel` selects and their points, reduced per workgroup: a crop's kept voxels, a carve's seen-through ones.  The
// predicate is evaluated for every slot (a carve's word load does not wait for the key's)
template <class SEL>
__global__ void __launch_bounds__(256) k_map_count(const unsigned long long *keys, const long long *pay, uint64_t cap, SEL sel,
                                                   unsigned long long *n_vox, unsigned long long *n_pts) {
  unsigned long long nv = 0, np = 0;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += stride) {
    const unsigned long long key = keys[i];
    const bool selected = sel(key, i);
    if (key >= kMapTomb || !selected) continue;
    ++nv;
    np += (unsigned long long)pay[4 * i + 3];
  }
  block_count<256>({nv, np}, {n_vox, n_pts});
}

// ---- removal in place (wc_map_carve_remove, wc_map_remove_keys: DESIGN 8.8) ----------------------------------------------------------
// k_map_count's pass with a store: the key word of every occupied slot that `sel` selects becomes a tombstone (a plain 8-byte store: no
// other lane of the launch reads a key, the selector looks at the carve's words), the voxel and its points are counted onto n_vox / n_pts
// and taken off the map's counters (the negated workgroup sums, added).  Payload and moment words stay as they are: no probe reaches
// them and a rehash does not carry them
template <class SEL>
__global__ void __launch_bounds__(256) k_map_erase(unsigned long long *keys, const long long *pay, uint64_t cap, SEL sel, unsigned long long *n_vox,
                                                   unsigned long long *n_pts, unsigned long long *ctr) {
  unsigned long long nv = 0, np = 0;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += stride) {
    const unsigned long long key = keys[i];
    const bool selected = sel(key, i);
    if (key >= kMapTomb || !selected) continue;
    keys[i] = kMapTomb;
    ++nv;
    np += (unsigned long long)pay[4 * i + 3];
  }
  block_count<256>({nv, np, 0ull - nv, 0ull - np}, {n_vox, n_pts, ctr + kCtrOcc, ctr + kCtrPts});
}

constexpr int kRemoveThreads = 256;
// one lane per voxel index (kx, ky, kz), grid-strided: the range test, the read-only probe chain, then a CAS of the key word to the
// tombstone - of the lanes that hold the same key exactly one sees it, the others (and an absent or out-of-range key) count as having
// removed nothing; the count load comes behind a won CAS.  A lane that probes past a slot another lane is removing reads the key or the
// tombstone: a foreign key either way
__global__ void __launch_bounds__(kRemoveThreads) k_map_remove_keys(const int32_t *in, uint64_t n, unsigned long long *keys, const long long *pay,
                                                                    unsigned long long mask, unsigned long long *ctr) {
  unsigned long long nv = 0, np = 0, nn = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kRemoveThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kRemoveThreads + threadIdx.x; i < n; i += stride) {
    const int kx = in[3 * i], ky = in[3 * i + 1], kz = in[3 * i + 2];
    const bool ok = kx > -kMapKeyOff && kx < kMapKeyOff && ky > -kMapKeyOff && ky < kMapKeyOff && kz > -kMapKeyOff && kz < kMapKeyOff;
    if (!ok) {
      ++nn;
      continue;
    }
    const unsigned long long key = map_pack(kx, ky, kz);
    unsigned long long h = map_hash(key) & mask;
    if (!map_find_from(keys, mask, key, h, keys[h]) || atomicCAS(&keys[h], key, kMapTomb) != key) {
      ++nn;
      continue;
    }
    ++nv;
    np += (unsigned long long)pay[4 * h + 3];
  }
  block_count<kRemoveThreads>({nv, np, nn, 0ull - nv, 0ull - np},
                              {ctr + kCtrRmVox, ctr + kCtrRmPts, ctr + kCtrRmNone, ctr + kCtrOcc, ctr + kCtrPts});
}

// ---- the exact state (wc_map_export_state, wc_map_absorb, wc_map_merge) -------------------------------------------------------------
constexpr int kStateThreads = 256;
constexpr unsigned kStateMaxCount = 1u << 30;  // a record's count: 1 .. 2^30 (the plain map's limit per voxel)
// the four (thirteen) integer sums of one voxel added to slot h: no-return 64-bit atomics (the slot may hold the key already, and two
// records of a call may carry the same key); integers, so no order matters
// (the two halves take register values: k_map_coarsen adds words it has re-based, map_add_sums words it loads)
__device__ __forceinline__ void map_add_pay(long long *pay, unsigned long long h, unsigned long long sx, unsigned long long sy, unsigned long long sz,
                                            unsigned long long cnt) {
  unsigned long long *p = (unsigned long long *)pay + 4 * h;
  atomicAdd(p + 0, sx);
  atomicAdd(p + 1, sy);
  atomicAdd(p + 2, sz);
  atomicAdd(p + 3, cnt);
}
__device__ __forceinline__ void map_add_mom(long long *mom, unsigned long long h, const unsigned long long (&w)[kMapMom]) {
  unsigned long long *pm = (unsigned long long *)mom + kMapMom * h;
#pragma unroll
  for (int j = 0; j < kMapMom; ++j) atomicAdd(pm + j, w[j]);
}
template <bool MOM>
__device__ __forceinline__ void map_add_sums(long long *pay, long long *mom, unsigned long long h, unsigned long long sx, unsigned long long sy,
                                             unsigned long long sz, unsigned long long cnt, const long long *src_mom) {
  map_add_pay(pay, h, sx, sy, sz, cnt);
  if constexpr (MOM) {
    unsigned long long w[kMapMom];
#pragma unroll
    for (int j = 0; j < kMapMom; ++j) w[j] = (unsigned long long)src_mom[j];  // (the nine loads leave before the first atomic)
    map_add_mom(mom, h, w);
  }
}

// state export, step 3: one lane per sorted voxel: the slot's payload as two 16-byte loads, the 40-byte wc_map_voxel as five 8-byte
// stores (key[0] is the low half of the first word: the host is little-endian, as the device), the nine moment words when asked for
__global__ void __launch_bounds__(kStateThreads) k_map_state(const unsigned long long *skeys, const uint32_t *sslots, uint64_t n, const long long *pay,
                                                             const long long *mom, wc_map_voxel *vox, long long *out_mom) {
  const uint64_t i = (uint64_t)blockIdx.x * kStateThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = skeys[i];
  const uint64_t slot = sslots[i];
  const longlong2 *p = (const longlong2 *)(pay + 4 * slot);
  const longlong2 p0 = p[0], p1 = p[1];
  const unsigned kx = (unsigned)map_unpack(key, 0), ky = (unsigned)map_unpack(key, 1), kz = (unsigned)map_unpack(key, 2);
  unsigned long long *o = (unsigned long long *)(vox + i);
  o[0] = (unsigned long long)kx | ((unsigned long long)ky << 32);
  o[1] = (unsigned long long)kz | ((unsigned long long)(unsigned)p1.y << 32);
  o[2] = (unsigned long long)p0.x;
  o[3] = (unsigned long long)p0.y;
  o[4] = (unsigned long long)p1.x;
  if (out_mom) {
#pragma unroll
    for (int w = 0; w < kMapMom; ++w) out_mom[kMapMom * i + w] = mom[kMapMom * slot + w];
  }
}

// absorb: grid-strided, one lane per record (five 8-byte loads); a record with a key out of range or a count outside 1 .. 2^30 is counted
// and not applied; map_slot finds or creates the voxel (its CAS settles lanes that create the same key), then the sums are added.  No
// LDS pre-aggregation: an exported state has distinct keys.  MOM: the map holds moments and in_mom is not NULL
template <bool MOM>
__global__ void __launch_bounds__(kStateThreads) k_map_absorb(const wc_map_voxel *vox, const long long *in_mom, uint64_t n, unsigned long long *keys,
                                                              long long *pay, long long *mom, unsigned long long mask, unsigned long long *ctr) {
  unsigned fresh = 0;
  unsigned long long n_pts = 0, n_rej = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kStateThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kStateThreads + threadIdx.x; i < n; i += stride) {
    const unsigned long long *r = (const unsigned long long *)(vox + i);
    const unsigned long long w0 = r[0], w1 = r[1], sx = r[2], sy = r[3], sz = r[4];
    const int kx = (int)(unsigned)w0, ky = (int)(unsigned)(w0 >> 32), kz = (int)(unsigned)w1;
    const unsigned cnt = (unsigned)(w1 >> 32);
    const bool ok = kx > -kMapKeyOff && kx < kMapKeyOff && ky > -kMapKeyOff && ky < kMapKeyOff && kz > -kMapKeyOff && kz < kMapKeyOff &&
                    cnt >= 1u && cnt <= kStateMaxCount;
    if (!ok) {
      ++n_rej;
      continue;
    }
    const unsigned long long h = map_slot(keys, mask, map_pack(kx, ky, kz), fresh);
    if (h == kMapEmpty) {  // (cannot happen: the growth policy left room for every record)
      atomicAdd(ctr + kCtrLost, 1ull);
      continue;
    }
    map_add_sums<MOM>(pay, mom, h, sx, sy, sz, (unsigned long long)cnt, MOM ? in_mom + kMapMom * i : nullptr);
    n_pts += cnt;
  }
  block_count<kStateThreads>({(unsigned long long)fresh, n_pts, n_rej}, {ctr + kCtrOcc, ctr + kCtrPts, ctr + kCtrRejCall});
}

// merge: one lane per slot of the source table, as k_map_rehash - but the destination may hold the key, so the sums are added, and the
// destination's voxel and point counters grow by what is new.  MOM: the destination holds moments (then the source does)
template <bool MOM>
__global__ void __launch_bounds__(kStateThreads) k_map_merge(const unsigned long long *skeys, const long long *spay, const long long *smom, uint64_t scap,
                                                             unsigned long long *keys, long long *pay, long long *mom, unsigned long long mask,
                                                             unsigned long long *ctr) {
  const uint64_t i = (uint64_t)blockIdx.x * kStateThreads + threadIdx.x;
  unsigned fresh = 0;
  unsigned long long n_pts = 0;
  const unsigned long long key = i < scap ? skeys[i] : kMapEmpty;
  if (key < kMapTomb) {
    const longlong2 *p = (const longlong2 *)(spay + 4 * i);
    const longlong2 p0 = p[0], p1 = p[1];
    const unsigned long long h = map_slot(keys, mask, key, fresh);
    if (h != kMapEmpty) {
      map_add_sums<MOM>(pay, mom, h, (unsigned long long)p0.x, (unsigned long long)p0.y, (unsigned long long)p1.x, (unsigned long long)p1.y,
                        MOM ? smom + kMapMom * i : nullptr);
      n_pts = (unsigned long long)p1.y;
    } else {  // (cannot happen: the growth policy left room for every voxel of the source)
      atomicAdd(ctr + kCtrLost, 1ull);
    }
  }
  block_count<kStateThreads>({(unsigned long long)fresh, n_pts}, {ctr + kCtrOcc, ctr + kCtrPts});
}

// coarsen (include/wildcat_hip.h: wc_map_coarsen): one lane per slot of the source table, as k_map_merge - but the key becomes
// K = floor(k / f) per axis and the sums are re-based from r(k, v) to r(K, V) in registers before they are added: the payload (two 16-byte
// loads) and the nine moment words are loaded before the first atomic, then one map_slot probe and four (thirteen) no-return atomic adds.
// Up to f^3 lanes add into one voxel; they sit at hashed slots of the source, so a workgroup has nothing to gather first.  D_a =
// (r(k_a, v) - r(K_a, V)) 2^32 is exact in fp64 (both on the 2^-10 m grid, below 2^23 m) and a multiple of 2^22, E_a = D_a >> 16.  All
// integer arithmetic is unsigned 64-bit, which wraps as the table's two's-complement adds do.  MOM: the destination holds moments (then the
// source does)
template <bool MOM>
__global__ void __launch_bounds__(kStateThreads) k_map_coarsen(const unsigned long long *skeys, const long long *spay, const long long *smom, uint64_t scap,
                                                               double v, double V, int f, unsigned long long *keys, long long *pay, long long *mom,
                                                               unsigned long long mask, unsigned long long *ctr) {
  const uint64_t i = (uint64_t)blockIdx.x * kStateThreads + threadIdx.x;
  unsigned fresh = 0;
  unsigned long long n_pts = 0;
  const unsigned long long key = i < scap ? skeys[i] : kMapEmpty;
  if (key < kMapTomb) {
    const longlong2 *p = (const longlong2 *)(spay + 4 * i);
    const longlong2 p0 = p[0], p1 = p[1];
    unsigned long long w[kMapMom];
    if constexpr (MOM) {
#pragma unroll
      for (int j = 0; j < kMapMom; ++j) w[j] = (unsigned long long)smom[kMapMom * i + j];
    }
    int K[3];
    unsigned long long D[3], E[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int k = map_unpack(key, a);
      K[a] = k / f - (k % f < 0 ? 1 : 0);  // floor(k / f): toward minus infinity
      const long long d = (long long)((map_ref(k, v) - map_ref(K[a], V)) * kMapUnit);
      D[a] = (unsigned long long)d;
      E[a] = (unsigned long long)(d >> 16);
    }
    const unsigned long long n = (unsigned long long)p1.y;
    const unsigned long long sx = (unsigned long long)p0.x + n * D[0], sy = (unsigned long long)p0.y + n * D[1],
                             sz = (unsigned long long)p1.x + n * D[2];
    if constexpr (MOM) {
      // M'_ab = M_ab + E_a U_b + E_b U_a + n E_a E_b with the source's U, then U'_a = U_a + n E_a
      const unsigned long long U[3] = {w[0], w[1], w[2]};
      constexpr int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
      for (int e = 0; e < 6; ++e) w[3 + e] += E[A[e]] * U[B[e]] + E[B[e]] * U[A[e]] + n * E[A[e]] * E[B[e]];
#pragma unroll
      for (int a = 0; a < 3; ++a) w[a] = U[a] + n * E[a];
    }
    const unsigned long long h = map_slot(keys, mask, map_pack(K[0], K[1], K[2]), fresh);
    if (h != kMapEmpty) {
      map_add_pay(pay, h, sx, sy, sz, n);
      if constexpr (MOM) map_add_mom(mom, h, w);
      n_pts = n;
    } else {  // (cannot happen: the table has room for every voxel of the source)
      atomicAdd(ctr + kCtrLost, 1ull);
    }
  }
  block_count<kStateThreads>({(unsigned long long)fresh, n_pts}, {ctr + kCtrOcc, ctr + kCtrPts});
}

// ---- a state under a rigid pose (include/wildcat_hip.h: wc_map_merge_moved, wc_map_move_state) -------------------------
constexpr unsigned long long kMovedBigCount = 1ull << 26;  // the most points a source voxel of a map with v > 2 m may hold (header: limits)
// one voxel's Gaussian - count n, sums S, moment words w (MOM) - moved by T: the key it lands in and its words relative to that voxel's
// reference point.  The kernel's and the host's one copy, every operation in the header's stated order (-ffp-contract=off: no fused
// multiply-add on either side).  false: the voxel is rejected and `o` is not to be used
struct map_moved_voxel {
  int K[3];
  unsigned long long S[3], w[kMapMom];
};
template <bool MOM>
__host__ __device__ __forceinline__ bool map_move_voxel(int kx, int ky, int kz, unsigned long long n, long long sx, long long sy, long long sz,
                                                        const unsigned long long (&w)[kMapMom], double v, const double (&T)[12],
                                                        map_moved_voxel &o) {
  const double dn = (double)n;
  // 1. the centroid, and where it goes
  const double cx = map_ref(kx, v) + ((double)sx / dn) * (1.0 / kMapUnit), cy = map_ref(ky, v) + ((double)sy / dn) * (1.0 / kMapUnit),
               cz = map_ref(kz, v) + ((double)sz / dn) * (1.0 / kMapUnit);
  const double px = ((T[0] * cx + T[1] * cy) + T[2] * cz) + T[3], py = ((T[4] * cx + T[5] * cy) + T[6] * cz) + T[7],
               pz = ((T[8] * cx + T[9] * cy) + T[10] * cz) + T[11];
  // 2. its voxel: the insert's rule; a non-finite coordinate or |K| >= 2^20 fails it
  if (!map_voxel_of(px, py, pz, v, o.K[0], o.K[1], o.K[2])) return false;
  if (v > 2.0 && n > kMovedBigCount) return false;
  // 3. the first sums: n times the centroid on the 2^-32 m grid
  const long long m[3] = {llrint((px - map_ref(o.K[0], v)) * kMapUnit), llrint((py - map_ref(o.K[1], v)) * kMapUnit),
                          llrint((pz - map_ref(o.K[2], v)) * kMapUnit)};
#pragma unroll
  for (int a = 0; a < 3; ++a) o.S[a] = n * (unsigned long long)m[a];
  if constexpr (MOM) {
    // 4. C = N / n with N_ab = n M_ab - U_a U_b in 128 bits, rounded once; C' = (R C) R^T; the words that give back n llrint(C')
    constexpr int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
    double c6[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const __int128 N = (__int128)(long long)n * (__int128)(long long)w[3 + e] - (__int128)(long long)w[A[e]] * (__int128)(long long)w[B[e]];
      const bool neg = N < 0;
      const double mag = map_u128_to_double(neg ? (unsigned __int128)(-N) : (unsigned __int128)N);
      c6[e] = (neg ? -mag : mag) / dn;
    }
    const double Cm[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    double Bm[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Bm[i][j] = (T[4 * i] * Cm[0][j] + T[4 * i + 1] * Cm[1][j]) + T[4 * i + 2] * Cm[2][j];
    }
    unsigned long long E[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      E[a] = (unsigned long long)((m[a] + 32768) >> 16);
      o.w[a] = n * E[a];
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const int i = A[e], j = B[e];
      const double c = (Bm[i][0] * T[4 * j] + Bm[i][1] * T[4 * j + 1]) + Bm[i][2] * T[4 * j + 2];
      o.w[3 + e] = (unsigned long long)llrint(c) + n * E[i] * E[j];
    }
  }
  return true;
}

// merge under a pose: one lane per slot of the source table, as k_map_coarsen - the payload (two 16-byte loads) and the nine moment words
// are loaded before the first atomic, map_move_voxel runs in registers, then one map_slot probe and four (thirteen) no-return atomic
// adds.  Lanes whose voxels land in one destination voxel sit at hashed slots of the source: nothing to gather first.  The pose and v
// travel in the kernel arguments.  Applied and rejected voxels and points go to the call's four counters, fresh voxels and applied
// points to the destination's own.  MOM: the destination holds moments (then the source does)
template <bool MOM>
__global__ void __launch_bounds__(kStateThreads) k_map_merge_moved(const unsigned long long *skeys, const long long *spay, const long long *smom,
                                                                   uint64_t scap, double v, map_pose P, unsigned long long *keys, long long *pay,
                                                                   long long *mom, unsigned long long mask, unsigned long long *ctr) {
  const uint64_t i = (uint64_t)blockIdx.x * kStateThreads + threadIdx.x;
  unsigned fresh = 0;
  unsigned long long n_vox = 0, n_pts = 0, r_vox = 0, r_pts = 0;
  const unsigned long long key = i < scap ? skeys[i] : kMapEmpty;
  if (key < kMapTomb) {
    const longlong2 *p = (const longlong2 *)(spay + 4 * i);
    const longlong2 p0 = p[0], p1 = p[1];
    unsigned long long w[kMapMom] = {};
    if constexpr (MOM) {
#pragma unroll
      for (int j = 0; j < kMapMom; ++j) w[j] = (unsigned long long)smom[kMapMom * i + j];
    }
    const unsigned long long n = (unsigned long long)p1.y;
    map_moved_voxel o;
    if (map_move_voxel<MOM>(map_unpack(key, 0), map_unpack(key, 1), map_unpack(key, 2), n, p0.x, p0.y, p1.x, w, v, P.T, o)) {
      const unsigned long long h = map_slot(keys, mask, map_pack(o.K[0], o.K[1], o.K[2]), fresh);
      if (h != kMapEmpty) {
        map_add_pay(pay, h, o.S[0], o.S[1], o.S[2], n);
        if constexpr (MOM) map_add_mom(mom, h, o.w);
        n_vox = 1, n_pts = n;
      } else {  // (cannot happen: the growth policy left room for every voxel of the source)
        atomicAdd(ctr + kCtrLost, 1ull);
      }
    } else {
      r_vox = 1, r_pts = n;
    }
  }
  block_count<kStateThreads>({(unsigned long long)fresh, n_pts, n_vox, n_pts, r_vox, r_pts},
                             {ctr + kCtrOcc, ctr + kCtrPts, ctr + kCtrMvVox, ctr + kCtrMvPts, ctr + kCtrMvRejVox, ctr + kCtrMvRejPts});
}

// ---- carving (wc_map_carve) -------------------------------------------------------------------------------------------------------
// what is the same for every ray of a call; the squares and the origin's voxel are formed once, on the host
struct map_ray_args {
  double o[3], v, min2, max2;
  int k0[3];      // the origin's voxel and whether it has one (map_voxel_of)
  unsigned k0_ok;
  unsigned shell, max_steps;
};
__device__ __forceinline__ int map_cheb(int ax, int ay, int az, int bx, int by, int bz) {
  return max(max(abs(ax - bx), abs(ay - by)), abs(az - bz));
}

// One ray of a call, as wc_map_carve and wc_map_raycast both define it (include/wildcat_hip.h): the walk's position k (k0 at first), the
// end voxel e, per axis the step s = sign(e - k0), u = 1 where the walk goes up (the face ahead is then k + 1) and the reciprocal i of the
// direction (of an axis that never is a candidate: never used; until map_ray_begin: the direction itself), and the number of steps M
struct map_ray {
  int kx, ky, kz, ex, ey, ez, sx, sy, sz, ux, uy, uz;
  double ix, iy, iz;
  unsigned M;
};
// the ray from the call's origin (ox, oy, oz) to the point P whose voxel is (ex, ey, ez): its k, e and M, and the direction d in r.i;
// false: the ray is not walked (the origin has no voxel, len2 outside the ranges or M > max_steps)
__device__ __forceinline__ bool map_ray_of(const map_ray_args &A, double ox, double oy, double oz, double px, double py, double pz, int ex, int ey, int ez,
                                           map_ray &r) {
  r.ix = px - ox, r.iy = py - oy, r.iz = pz - oz;
  const double len2 = (r.ix * r.ix + r.iy * r.iy) + r.iz * r.iz;
  r.kx = A.k0[0], r.ky = A.k0[1], r.kz = A.k0[2], r.ex = ex, r.ey = ey, r.ez = ez;
  r.M = (unsigned)abs(ex - r.kx) + (unsigned)abs(ey - r.ky) + (unsigned)abs(ez - r.kz);
  return A.k0_ok != 0u && len2 >= A.min2 && len2 <= A.max2 && r.M <= A.max_steps;
}
// ... and, for a ray that is walked, what its steps need: s, u and the reciprocals 1.0 / d, formed once per ray
__device__ __forceinline__ void map_ray_begin(map_ray &r) {
  r.sx = r.ex > r.kx ? 1 : (r.ex < r.kx ? -1 : 0), r.sy = r.ey > r.ky ? 1 : (r.ey < r.ky ? -1 : 0), r.sz = r.ez > r.kz ? 1 : (r.ez < r.kz ? -1 : 0);
  r.ux = r.ex > r.kx ? 1 : 0, r.uy = r.ey > r.ky ? 1 : 0, r.uz = r.ez > r.kz ? 1 : 0;
  r.ix = 1.0 / r.ix, r.iy = 1.0 / r.iy, r.iz = 1.0 / r.iz;
}
// the parameter at which a ray crosses the face ahead of voxel index k on one axis: the face's coordinate comes from the integer every
// time, so nothing drifts
__device__ __forceinline__ double map_face_t(int k, int u, double v, double o, double inv) { return ((double)(k + u) * v - o) * inv; }
// the step rule: among the axes that have not arrived, the one whose next face is crossed first; a later axis wins only on a strictly
// smaller parameter.  The position moves when `live`; returns the axis
__device__ __forceinline__ int map_ray_step(map_ray &r, double v, double ox, double oy, double oz, bool live) {
  const bool cx = r.kx != r.ex, cy = r.ky != r.ey, cz = r.kz != r.ez;
  const double tx = map_face_t(r.kx, r.ux, v, ox, r.ix), ty = map_face_t(r.ky, r.uy, v, oy, r.iy), tz = map_face_t(r.kz, r.uz, v, oz, r.iz);
  int ax = cx ? 0 : (cy ? 1 : 2);
  double bt = cx ? tx : (cy ? ty : tz);
  if (cx && cy && ty < bt) ax = 1, bt = ty;
  if ((cx || cy) && cz && tz < bt) ax = 2, bt = tz;
  r.kx += (live && ax == 0) ? r.sx : 0;
  r.ky += (live && ax == 1) ? r.sy : 0;
  r.kz += (live && ax == 2) ? r.sz : 0;
  return ax;
}

// One lane per point (include/wildcat_hip.h: wc_map_carve states every expression).  The end voxel's word gets bit 31; a used ray then
// walks its M voxel steps, known before the loop, B at a time: the B positions, their keys, hashes and shell tests come first - the next
// voxel does not depend on what a probe finds - with the B first-slot key loads issued as they are formed; only then are the loads looked
// at, the chains followed and the words of the occupied voxels incremented (no-return atomics).  |k - ke| shrinks monotonically on
// every axis, so the first position inside the shell ends the walk: nothing after it is seen through.  k^(M) = ke never is, and is not
// visited.  Every index below is a compile-time constant (no scratch); the axis is chosen and applied with selects (map_ray_step).
template <int B>
__global__ void __launch_bounds__(kCarveThreads) k_map_carve(wc_points pts, map_ray_args A, const unsigned long long *keys, unsigned long long mask,
                                                             unsigned *words, unsigned long long *cctr) {
  unsigned long long n_used = 0, n_skip = 0, n_steps = 0;
  const double v = A.v, ox = A.o[0], oy = A.o[1], oz = A.o[2];
  const int shell = (int)A.shell;
  const uint64_t stride = (uint64_t)gridDim.x * kCarveThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kCarveThreads + threadIdx.x; i < pts.n; i += stride) {
    const float *f = (const float *)((const char *)pts.xyz + i * pts.xyz_stride);
    const double px = (double)f[0], py = (double)f[1], pz = (double)f[2];
    int kex, key_, kez;
    if (!map_voxel_of(px, py, pz, v, kex, key_, kez)) {
      ++n_skip;
      continue;
    }
    {  // the end mark, whether or not the ray is used
      const unsigned long long ekey = map_pack(kex, key_, kez);
      unsigned long long es = map_hash(ekey) & mask;
      if (map_find_from(keys, mask, ekey, es, keys[es])) atomicOr(&words[es], kCarveEnd);
    }
    map_ray r;
    if (!map_ray_of(A, ox, oy, oz, px, py, pz, kex, key_, kez, r)) {
      ++n_skip;
      continue;
    }
    ++n_used;
    n_steps += r.M;
    map_ray_begin(r);
    for (unsigned base = 0; base < r.M; base += B) {  // a counted loop: at most ceil(M / B) rounds
      if (map_cheb(r.kx, r.ky, r.kz, kex, key_, kez) <= shell) break;
      unsigned long long key[B], h[B], cur[B];
#pragma unroll
      for (int j = 0; j < B; ++j) {
        const bool live = base + j < r.M;
        const bool thru = live && map_cheb(r.kx, r.ky, r.kz, kex, key_, kez) > shell;
        // (a step that is not seen through: the empty mark, which the settling loop skips; its load reads slot 0 and is dropped)
        key[j] = thru ? map_pack(r.kx, r.ky, r.kz) : kMapEmpty;
        h[j] = thru ? map_hash(key[j]) & mask : 0ull;
        cur[j] = keys[h[j]];
        map_ray_step(r, v, ox, oy, oz, live);
      }
#pragma unroll
      for (int j = 0; j < B; ++j) {
        if (key[j] == kMapEmpty) continue;
        if (map_find_from(keys, mask, key[j], h[j], cur[j])) atomicAdd(&words[h[j]], 1u);
      }
    }
  }
  block_count<kCarveThreads>({n_used, n_skip, n_steps}, {cctr + kCarveUsed, cctr + kCarveSkip, cctr + kCarveSteps});
}

// ---- ray casting (wc_map_raycast) -------------------------------------------------------------------------------------------------
// One lane per ray (include/wildcat_hip.h: wc_map_raycast states every expression), the carve's ray (map_ray_of, map_ray_step) with another
// ending: the M + 1 positions k^(0) .. k^(M) are taken B at a time - keys, hashes and tested-flags of a batch first, its first-slot key
// loads issued as they are formed; an untested position carries the empty mark - and only then looked at in ascending order.  Read-only: no
// atomics but the counters'.  A lane is done at its first hit: a tested position whose voxel is there with at least min_points points
// (the count is a dependent load behind the chain; with min_points = 1 the first voxel found is the hit, so it is loaded once per ray).
// The Chebyshev distance to ke never grows, so a batch that begins inside the end shell ends the walk.  Of a batch only the axis by which
// each position was entered is kept, two bits each in one word: the hit's t is formed again from the hit voxel's index, the very
// expression the step rule compared (map_face_t).  Every register-array index and shift is a compile-time constant; the loop is counted.
template <int B>
__global__ void __launch_bounds__(kCastThreads) k_map_raycast(wc_points pts, map_ray_args A, unsigned first_step, unsigned min_points,
                                                              const unsigned long long *keys, const long long *pay, unsigned long long mask,
                                                              wc_map_ray_hit *hits, unsigned long long *cctr) {
  static_assert(B <= 16, "two bits per position of a batch in one 32-bit word");
  unsigned long long n_cast = 0, n_skip = 0, n_hit = 0, n_tested = 0;
  const double v = A.v, ox = A.o[0], oy = A.o[1], oz = A.o[2];
  const int shell = (int)A.shell;
  const uint64_t stride = (uint64_t)gridDim.x * kCastThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kCastThreads + threadIdx.x; i < pts.n; i += stride) {
    const float *f = (const float *)((const char *)pts.xyz + i * pts.xyz_stride);
    const double px = (double)f[0], py = (double)f[1], pz = (double)f[2];
    int kex, key_, kez;
    map_ray r;
    const bool cast = map_voxel_of(px, py, pz, v, kex, key_, kez) && map_ray_of(A, ox, oy, oz, px, py, pz, kex, key_, kez, r);
    unsigned tested = 0, hstep = 0, hax = 3, hcount = 0;
    unsigned long long hkey = kMapEmpty, hslot = 0;
    if (cast) {
      map_ray_begin(r);
      int ax_in = 3;  // the axis by which the position at hand was entered; 3: it is k^(0)
      for (unsigned base = 0; base <= r.M; base += B) {  // a counted loop: at most M / B + 1 rounds
        if (hkey != kMapEmpty || map_cheb(r.kx, r.ky, r.kz, kex, key_, kez) < shell) break;
        unsigned long long key[B], h[B], cur[B];
        unsigned axes = 0;
#pragma unroll
        for (int j = 0; j < B; ++j) {
          const unsigned at = base + j;
          const bool test = at <= r.M && at >= first_step && map_cheb(r.kx, r.ky, r.kz, kex, key_, kez) >= shell;
          // (a position that is not tested: the empty mark, which the loop below skips; its load reads slot 0 and is dropped)
          key[j] = test ? map_pack(r.kx, r.ky, r.kz) : kMapEmpty;
          h[j] = test ? map_hash(key[j]) & mask : 0ull;
          cur[j] = keys[h[j]];
          axes |= (unsigned)ax_in << (2 * j);
          ax_in = map_ray_step(r, v, ox, oy, oz, at < r.M);
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
          if (hkey != kMapEmpty || key[j] == kMapEmpty) continue;
          ++tested;
          if (!map_find_from(keys, mask, key[j], h[j], cur[j])) continue;
          const unsigned c = (unsigned)pay[4 * h[j] + 3];
          if (c >= min_points) hkey = key[j], hslot = h[j], hcount = c, hstep = base + j, hax = (axes >> (2 * j)) & 3u;
        }
      }
    }
    const bool hit = hkey != kMapEmpty;
    n_cast += cast ? 1u : 0u, n_skip += cast ? 0u : 1u, n_hit += hit ? 1u : 0u, n_tested += tested;
    float cx = 0.f, cy = 0.f, cz = 0.f;
    int hx = 0, hy = 0, hz = 0;
    double t = __builtin_inf();
    if (hit) {
      const longlong2 *p = (const longlong2 *)(pay + 4 * hslot);
      const longlong2 p0 = p[0], p1 = p[1];
      const double cnt = (double)hcount;
      hx = map_unpack(hkey, 0), hy = map_unpack(hkey, 1), hz = map_unpack(hkey, 2);
      cx = map_centroid(hx, v, p0.x, cnt), cy = map_centroid(hy, v, p0.y, cnt), cz = map_centroid(hz, v, p1.x, cnt);
      // the face through which the step into the hit voxel went: the one ahead of the voxel before it on that axis
      const double tx = map_face_t(hx - r.sx, r.ux, v, ox, r.ix), ty = map_face_t(hy - r.sy, r.uy, v, oy, r.iy),
                   tz = map_face_t(hz - r.sz, r.uz, v, oz, r.iz);
      t = hax == 0u ? tx : (hax == 1u ? ty : (hax == 2u ? tz : 0.0));
    }
    // the 48-byte record as six 8-byte stores (the record is 8-aligned)
    uint2 *o = (uint2 *)(hits + i);
    o[0] = make_uint2(__float_as_uint(cx), __float_as_uint(cy));
    o[1] = make_uint2(__float_as_uint(cz), hcount);
    o[2] = make_uint2((unsigned)hx, (unsigned)hy);
    o[3] = make_uint2((unsigned)hz, cast ? 0u : 1u);
    ((double *)o)[4] = t;
    o[5] = make_uint2(hstep, tested);
  }
  block_count<kCastThreads>({n_cast, n_skip, n_hit, n_tested}, {cctr + kCastCast, cctr + kCastSkip, cctr + kCastHits, cctr + kCastTested});
}

// ---- connected components (wc_map_components, wc_map_remove_small: DESIGN 8.14) -------------------------------------------------------
constexpr int kCcThreads = 256;
constexpr uint32_t kCcNone = 0xFFFFFFFFu;  // WC_MAP_NO_COMPONENT: in the per-slot index and the parent array, a voxel that is not a node
constexpr int kCcNodes = 0, kCcComps = 16, kCcLargest = 32, kCcErr = 48, kCcRmComps = 64, kCcRmVox = 80, kCcRmPts = 96,
              kCcCtrWords = 112;  // u64 word of each of the calls' counters
// the 13 lexicographically negative offsets of the 27-neighbourhood: the 3 faces, then the 6 edges, then the 4 corners, so that
// connectivity 6 / 18 / 26 is the first 3 / 9 / 13 of them.  The same table on the host (wc_map_label_keys)
__host__ __device__ constexpr int cc_off(int j, int a) {
  constexpr int t[13][3] = {{-1, 0, 0},  {0, -1, 0},  {0, 0, -1},  {-1, -1, 0}, {-1, 1, 0},  {-1, 0, -1}, {-1, 0, 1},
                            {0, -1, -1}, {0, -1, 1},  {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};
  return t[j][a];
}
__host__ __device__ constexpr int cc_lower(uint32_t connectivity) { return connectivity == 6 ? 3 : (connectivity == 18 ? 9 : 13); }
__host__ __device__ __forceinline__ bool cc_in_range(int k) { return k > -kMapKeyOff && k < kMapKeyOff; }

// The parent array inside the link launch: EVERY access is an agent-scope atomic (a load that bypasses the CU's L1, a compare-and-swap or a
// minimum at L2) - workgroups read here the words other workgroups write in the same launch, and a plain load could follow a stale L1 line
// for ever
__device__ __forceinline__ uint32_t cc_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// Unites the trees of a and b.  Invariant of the array: parent[x] <= x, and only a root (parent[x] == x) is ever hooked, under a smaller
// root - parents only ever decrease, so the root that remains of a component is its smallest index.  `a` is ANY member of the lane's own
// component (the lane's entry at first) and comes back as the root the call ended on, where the lane's next call starts: in a settled
// region the neighbour's parent IS that root, and the call is one load that does not touch the root's own word - the one word every lane
// of a large component would otherwise load twice per neighbour.  No lane waits for another: `steps` counts every load and every
// compare-and-swap of the call against `budget` (8 n + 64, derived below); false: the budget ran out
__device__ __forceinline__ bool cc_unite(uint32_t *parent, uint32_t &a, uint32_t b, unsigned long long budget) {
  unsigned long long steps = 0;
  while (true) {
    // the two walks to a root, b's first.  Termination: every iteration replaces x by parent[x] < x, so a walk from x takes at most x
    // iterations whatever other lanes do meanwhile (they only lower parents); on the way x's link is shortened to its grandparent (a
    // minimum: the word only decreases and keeps pointing at an ancestor).  b's walk ends early when it meets a: one component already
#pragma unroll
    for (int w = 1; w >= 0; --w) {
      uint32_t x = w ? b : a;
      uint32_t p = cc_load(parent + x);
      ++steps;
      while (p != x && !(w && p == a)) {
        if (++steps > budget) return false;
        const uint32_t g = cc_load(parent + p);
        if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p, p = g;
      }
      if (w && p == a) return true;  // (a is an ancestor of b, or b itself)
      if (w)
        b = x;
      else
        a = x;
    }
    if (a == b) return true;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
      a = lo;
      return true;
    }
    // a failed compare-and-swap means another lane lowered parent[hi] (seen < hi): hi is no root any more.  The pair goes on from
    // (seen, lo), strictly below (hi, lo): over the whole call a + b decreases with every walk step and every failure, so there are at
    // most a + b <= 2 n of them, each with at most three loads and one compare-and-swap - the budget of 8 n + 64 is never reached
    if (++steps > budget) return false;
    a = seen, b = lo;
  }
}

// the per-slot index and the parent array: export entry i of a node into idx[its slot] and parent[i]; kCcNone for an occupied voxel with
// fewer than min_points points.  Only occupied slots' words are written, and only those are ever read (a probe ends on the key)
__global__ void __launch_bounds__(kCcThreads) k_map_cc_index(const uint32_t *sslots, uint64_t n, const long long *pay, unsigned min_points, uint32_t *idx,
                                                             uint32_t *parent, unsigned long long *cctr) {
  unsigned long long nodes = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kCcThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; i < n; i += stride) {
    const uint32_t slot = sslots[i];
    const bool node = (unsigned long long)pay[4 * (uint64_t)slot + 3] >= min_points;
    const uint32_t w = node ? (uint32_t)i : kCcNone;
    idx[slot] = w;
    parent[i] = w;
    nodes += node;
  }
  block_count<kCcThreads>({nodes}, {cctr + kCcNodes});
}

// one lane per export entry, grid-strided: the NB lower neighbours of a node - their keys, hashes and range tests, their first-slot key
// loads issued together (as k_map_nearest does per plane of nine), then the chains (read-only: the table is not written here), one word
// of the index per neighbour found, and a cc_unite per neighbour that is a node.  Every register array is indexed by the unrolled loops'
// constants.  A lane whose cc_unite runs out of budget counts itself in *err and leaves: the host reports WC_ERR_INTERNAL
template <int NB>
__global__ void __launch_bounds__(kCcThreads) k_map_cc_link(const unsigned long long *skeys, uint64_t n, const unsigned long long *keys,
                                                            unsigned long long mask, const uint32_t *idx, uint32_t *parent,
                                                            unsigned long long budget, unsigned long long *err) {
  const uint64_t stride = (uint64_t)gridDim.x * kCcThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; i < n; i += stride) {
    if (cc_load(parent + i) == kCcNone) continue;  // (not a node: the word never changes)
    const unsigned long long key = skeys[i];
    const int kx = map_unpack(key, 0), ky = map_unpack(key, 1), kz = map_unpack(key, 2);
    unsigned long long nk[NB], c[NB];
    uint32_t h[NB];
    uint32_t mine = (uint32_t)i;  // (a member of this lane's component: cc_unite moves it to the root it ends on)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int x = kx + cc_off(j, 0), y = ky + cc_off(j, 1), z = kz + cc_off(j, 2);
      const bool ok = cc_in_range(x) && cc_in_range(y) && cc_in_range(z);  // (a neighbour outside the key range does not exist: no field wraps)
      nk[j] = map_pack(x, y, z);
      h[j] = (uint32_t)(map_hash(nk[j]) & mask);
      c[j] = ok ? keys[h[j]] : kMapEmpty;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (c[j] == kMapEmpty) continue;  // (out of range, or an empty first slot: absent)
      unsigned long long hh = h[j];
      if (!map_find_from(keys, mask, nk[j], hh, c[j])) continue;
      const uint32_t other = idx[hh];
      if (other == kCcNone) continue;
      if (!cc_unite(parent, mine, other, budget)) {
        atomicAdd(err, 1ull);
        return;
      }
    }
  }
}

// a separate launch: the parent array is only read here (what the link launch wrote), so plain loads.  root[i] = the root of i's tree, its
// component's smallest index; flag[i] = 1 for a root; kCcNone / 0 for a voxel that is not a node.  The walk strictly decreases: at most
// i steps; the bound guards a broken array
__global__ void __launch_bounds__(kCcThreads) k_map_cc_flatten(const uint32_t *parent, uint64_t n, uint32_t *root, uint32_t *flag,
                                                               unsigned long long *cctr) {
  unsigned long long roots = 0, bad = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kCcThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; i < n; i += stride) {
    uint32_t x = (uint32_t)i, p = parent[i];
    if (p == kCcNone) {
      root[i] = kCcNone, flag[i] = 0;
      continue;
    }
    uint64_t steps = 0;
    while (p != x && p < x && steps <= n) x = p, p = parent[x], ++steps;
    bad += p != x;
    root[i] = x;
    flag[i] = x == (uint32_t)i;
    roots += x == (uint32_t)i;
  }
  block_count<kCcThreads>({roots, bad}, {cctr + kCcComps, cctr + kCcErr});
}

__global__ void __launch_bounds__(kCcThreads) k_map_cc_clear(wc_map_component *comps, uint64_t C) {
  const uint64_t stride = (uint64_t)gridDim.x * kCcThreads;
  for (uint64_t c = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; c < C; c += stride) {
    wc_map_component r;
    r.first = 0, r.voxels = 0, r.points = 0;
    r.kmin[0] = r.kmin[1] = r.kmin[2] = INT32_MAX;
    r.kmax[0] = r.kmax[1] = r.kmax[2] = INT32_MIN;
    comps[c] = r;
  }
}

// the sums and bounds a wavefront holds for ONE component, lane by lane, until cc_flush reduces them across the wavefront and lane 0
// issues the eight integer atomics
struct cc_acc {
  unsigned vox = 0;
  unsigned long long pts = 0;
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
};
__device__ __forceinline__ void cc_flush(cc_acc &acc, uint32_t comp, wc_map_component *comps, unsigned lane) {
  const unsigned vox = wave_sum(acc.vox);
  const unsigned long long pts = wave_sum(acc.pts);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o; o >>= 1) acc.lo[a] = min(acc.lo[a], __shfl_down(acc.lo[a], o)), acc.hi[a] = max(acc.hi[a], __shfl_down(acc.hi[a], o));
  }
  if (lane == 0 && vox) {
    wc_map_component *c = comps + comp;
    atomicAdd(&c->voxels, vox);
    atomicAdd((unsigned long long *)&c->points, pts);
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicMin(&c->kmin[a], acc.lo[a]), atomicMax(&c->kmax[a], acc.hi[a]);
  }
  acc = cc_acc{};
}
// labels and records: num[] is the exclusive scan of the root flags, so a component's number is num[its root].  Every wavefront takes a
// CONTIGUOUS run of 64-entry tiles of the export order.  While the nodes of its tiles all lie in one component (the rule in key order:
// a wall is thousands of consecutive entries) each lane adds its own entries up in registers, and the wavefront issues its eight
// integer atomics once per run of tiles (Guideline 12: a large component's record is ONE line, and an atomic per tile on it was the
// whole cost of the call); a tile with nodes of several components issues one set per distinct component.  Integers: no order matters.  Reads only
// what earlier launches wrote
__global__ void __launch_bounds__(kCcThreads) k_map_cc_stats(const unsigned long long *skeys, const uint32_t *sslots, uint64_t n, const long long *pay,
                                                             const uint32_t *root, const uint32_t *num, uint32_t *label, int32_t *keys_out,
                                                             wc_map_component *comps) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t wave = ((uint64_t)blockIdx.x * kCcThreads + threadIdx.x) >> 6, waves = (uint64_t)gridDim.x * (kCcThreads / 64);
  const uint64_t tiles = (n + 63) / 64, per = (tiles + waves - 1) / waves;
  const uint64_t t_end = wave * per + per < tiles ? wave * per + per : tiles;
  cc_acc acc;
  uint32_t cur = kCcNone;  // (the component the accumulators belong to: the same in every lane)
  // (the bounds are the wavefront's: every lane of a wavefront takes the same trips, so the cross-lane operations are whole)
  for (uint64_t t = wave * per; t < t_end; ++t) {
    const uint64_t i = t * 64 + lane;
    uint32_t comp = kCcNone;
    unsigned long long cnt = 0;
    int k[3] = {0, 0, 0};
    if (i < n) {
      const unsigned long long key = skeys[i];
      const uint32_t r = root[i];
#pragma unroll
      for (int a = 0; a < 3; ++a) k[a] = map_unpack(key, a);
      if (keys_out) keys_out[3 * i] = k[0], keys_out[3 * i + 1] = k[1], keys_out[3 * i + 2] = k[2];
      if (r != kCcNone) {
        comp = num[r];
        cnt = (unsigned long long)pay[4 * (uint64_t)sslots[i] + 3];
        if (r == (uint32_t)i) comps[comp].first = r;  // (the one writer of this word)
      }
      if (label) label[i] = comp;
    }
    const unsigned long long nodes = __ballot(comp != kCcNone);
    if (!nodes) continue;
    const uint32_t c0 = (uint32_t)__shfl((int)comp, __ffsll((long long)nodes) - 1);
    const bool one = __all(comp == c0 || comp == kCcNone);
    if (cur != kCcNone && !(one && c0 == cur)) {
      cc_flush(acc, cur, comps, lane);
      cur = kCcNone;
    }
    if (one) {
      cur = c0;
      if (comp != kCcNone) {
        acc.vox += 1, acc.pts += cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) acc.lo[a] = min(acc.lo[a], k[a]), acc.hi[a] = max(acc.hi[a], k[a]);
      }
    } else {
      // several components in one tile (the rings a spinning lidar leaves on a floor interleave in key order): one reduction and one
      // set of atomics per DISTINCT component of the tile, not per node - a loop of at most 64 wavefront-uniform trips
      unsigned long long left = nodes;
      while (left) {
        const uint32_t c = (uint32_t)__shfl((int)comp, __ffsll((long long)left) - 1);
        const bool mine = comp == c;
        cc_acc part;
        if (mine) {
          part.vox = 1, part.pts = cnt;
#pragma unroll
          for (int a = 0; a < 3; ++a) part.lo[a] = part.hi[a] = k[a];
        }
        cc_flush(part, c, comps, lane);
        left &= ~__ballot(mine);
      }
    }
  }
  if (cur != kCcNone) cc_flush(acc, cur, comps, lane);
}

// over the C records: the largest component's voxels; with sel != NULL (wc_map_remove_small) sel[c] = 1 for a component below a
// threshold that is switched on, and their number
__global__ void __launch_bounds__(kCcThreads) k_map_cc_select(const wc_map_component *comps, uint64_t C, uint32_t min_voxels,
                                                              unsigned long long min_points, uint32_t *sel, unsigned long long *cctr) {
  unsigned long long largest = 0, gone = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kCcThreads;
  for (uint64_t c = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; c < C; c += stride) {
    const uint32_t v = comps[c].voxels;
    const unsigned long long p = comps[c].points;
    largest = largest > v ? largest : (unsigned long long)v;
    if (sel) {
      const bool s = (min_voxels && v < min_voxels) || (min_points && p < min_points);
      sel[c] = s;
      gone += s;
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const unsigned long long other = __shfl_down(largest, o);
    largest = largest > other ? largest : other;
  }
  if ((threadIdx.x & 63) == 0 && largest) atomicMax(cctr + kCcLargest, largest);
  block_count<kCcThreads>({gone}, {cctr + kCcRmComps});
}

// wc_map_remove_small's pass over the export entries: the slot of every voxel of a selected component (and, with drop_sparse, of every
// voxel that is not a node) gets the tombstone by a plain 8-byte store - no lane of this launch reads a key -, and the counters move as
// k_map_erase moves them
__global__ void __launch_bounds__(kCcThreads) k_map_cc_erase(const uint32_t *sslots, uint64_t n, const uint32_t *root, const uint32_t *num,
                                                             const uint32_t *sel, unsigned drop_sparse, unsigned long long *keys, const long long *pay,
                                                             unsigned long long *cctr, unsigned long long *ctr) {
  unsigned long long nv = 0, np = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kCcThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; i < n; i += stride) {
    const uint32_t r = root[i];
    const bool gone = r == kCcNone ? drop_sparse != 0 : sel[num[r]] != 0;
    if (!gone) continue;
    const uint64_t slot = sslots[i];
    keys[slot] = kMapTomb;
    ++nv;
    np += (unsigned long long)pay[4 * slot + 3];
  }
  block_count<kCcThreads>({nv, np, 0ull - nv, 0ull - np}, {cctr + kCcRmVox, cctr + kCcRmPts, ctr + kCtrOcc, ctr + kCtrPts});
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int map_alloc(wc_ctx *ctx, void **p, size_t bytes) {
  *p = nullptr;
  if (ctx->pool_ok && hipMallocFromPoolAsync(p, bytes, ctx->pool, ctx->stream) == hipSuccess) return WC_OK;
  (void)hipGetLastError();
  *p = nullptr;
  WC_HIP(ctx, hipMalloc(p, bytes));
  return WC_OK;
}
void map_free(wc_ctx *ctx, void *p) {
  if (!p) return;
  if (ctx->pool_ok) {  // (pool blocks and plain blocks alike: hipFreeAsync releases either, in stream order)
    if (hipFreeAsync(p, ctx->stream) == hipSuccess) return;
    (void)hipGetLastError();
  }
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(p);
}
// a table of `cap` slots made empty (empty keys, zero payload; mom: NULL for a plain map), enqueued on the ctx stream
int map_clear_table(wc_ctx *ctx, uint64_t cap, unsigned long long *keys, long long *pay, long long *mom) {
  WC_HIP(ctx, hipMemsetAsync(keys, 0xFF, cap * 8, ctx->stream));
  WC_HIP(ctx, hipMemsetAsync(pay, 0, cap * 32, ctx->stream));
  if (mom) WC_HIP(ctx, hipMemsetAsync(mom, 0, cap * 8 * kMapMom, ctx->stream));
  return WC_OK;
}
// a fresh, empty table of `cap` slots
// (moments: the nine extra words per slot of a WC_MAP_MOMENTS map; *mom = NULL otherwise)
int map_table(wc_ctx *ctx, uint64_t cap, bool moments, unsigned long long **keys, long long **pay, long long **mom) {
  *mom = nullptr;
  WC_TRY(map_alloc(ctx, (void **)keys, cap * 8));
  int rc = map_alloc(ctx, (void **)pay, cap * 32);
  if (rc == WC_OK && moments) {
    rc = map_alloc(ctx, (void **)mom, cap * 8 * kMapMom);
    if (rc != WC_OK) {
      map_free(ctx, *pay);
      *pay = nullptr;
    }
  }
  if (rc != WC_OK) {
    map_free(ctx, *keys);
    *keys = nullptr;
    return rc;
  }
  return map_clear_table(ctx, cap, *keys, *pay, *mom);
}
// the map's table replaced by one of `cap` slots that holds the occupied slots `sel` selects: the new table, the rehash into it, the
// old one freed (in stream order, behind the rehash)
template <class SEL>
int map_replace_table(wc_ctx *ctx, wc_map *m, uint64_t cap, SEL sel) {
  unsigned long long *keys = nullptr;
  long long *pay = nullptr, *mom = nullptr;
  WC_TRY(map_table(ctx, cap, m->mom != nullptr, &keys, &pay, &mom));
  k_map_rehash<SEL><<<(unsigned)((m->cap + 255) / 256), 256, 0, ctx->stream>>>(m->keys, m->pay, m->mom, m->cap, keys, pay, mom, cap - 1, sel);
  WC_HIP(ctx, hipGetLastError());
  map_free(ctx, m->keys);
  map_free(ctx, m->pay);
  map_free(ctx, m->mom);
  m->keys = keys, m->pay = pay, m->mom = mom, m->cap = cap;
  return WC_OK;
}
// one launch of the insert: PTS consecutive points per lane, tiles of kMapThreads * PTS points
template <bool MOM, int PTS>
void map_launch_insert(wc_ctx *ctx, wc_map *m, const wc_points &pts) {
  const uint64_t tiles = (pts.n + kMapThreads * PTS - 1) / (kMapThreads * PTS);
  const unsigned grid = (unsigned)std::min<uint64_t>(tiles, (uint64_t)4 * m->cus);
  k_map_insert<MOM, PTS><<<grid, kMapThreads, 0, ctx->stream>>>(pts, m->voxel, m->keys, m->pay, m->mom, m->cap - 1, m->ctr);
}
// the occupied-slot bound of the growth policy; takes a completed read-back into account without waiting for one
uint64_t map_bound(wc_map *m) {
  if (m->ctr_pending && hipEventQuery(m->ev_ctr) == hipSuccess) {
    m->occ_known = m->h_ctr[kCtrOcc];
    m->pts_since = m->pts_after_copy;
    m->ctr_pending = false;
  }
  return m->occ_known + m->pts_since;
}
int map_sync_counters(wc_ctx *ctx, wc_map *m) {
  WC_HIP(ctx, hipMemcpyAsync(m->h_ctr, m->ctr, kCtrWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  m->occ_known = m->h_ctr[kCtrOcc];
  m->pts_since = 0;
  m->ctr_pending = false;
  if (m->h_ctr[kCtrLost]) return wc_fail(ctx, WC_ERR_HIP, "wc_map: %llu voxels found no slot (growth invariant broken)", m->h_ctr[kCtrLost]);
  return WC_OK;
}
bool map_ok(const wc_ctx *ctx, const wc_map *m) { return ctx && m && m->ctx == ctx; }
// a cloud the kernels can read: not null and, unless it is empty, float triples at a 4-byte-aligned address, a stride of at least 12 bytes
// that is a multiple of 4
bool map_points_ok(const wc_points *p) {
  return p && (p->n == 0 || (p->xyz && p->xyz_stride >= 12 && p->xyz_stride % 4 == 0 && (uintptr_t)p->xyz % 4 == 0));
}

}  // namespace

extern "C" int wc_map_create(wc_ctx *ctx, double voxel, uint64_t reserve_voxels, wc_map **out) {
  return wc_map_create_ex(ctx, voxel, reserve_voxels, 0u, out);
}

extern "C" int wc_map_create_ex(wc_ctx *ctx, double voxel, uint64_t reserve_voxels, uint32_t flags, wc_map **out) {
  wc_dev_guard dg_(ctx);
  if (!ctx || !out || !(voxel >= 0.01 && voxel <= 4.0) || reserve_voxels > ((uint64_t)1 << 31) || (flags & ~(uint32_t)WC_MAP_MOMENTS))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument (0.01 <= voxel <= 4.0, reserve_voxels <= 2^31, flags: WC_MAP_MOMENTS)",
                   __func__);
  *out = nullptr;
  wc_map *m = new wc_map;
  m->ctx = ctx;
  m->voxel = voxel;
  m->flags = flags;
  m->cap = pow2_at_least(2 * (reserve_voxels ? reserve_voxels : 1));
  if (hipDeviceGetAttribute(&m->cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || m->cus <= 0) m->cus = 256;
  int rc = map_table(ctx, m->cap, (flags & WC_MAP_MOMENTS) != 0, &m->keys, &m->pay, &m->mom);
  if (rc == WC_OK) rc = map_alloc(ctx, (void **)&m->ctr, kCtrWords * 8);
  if (rc == WC_OK && hipMemsetAsync(m->ctr, 0, kCtrWords * 8, ctx->stream) != hipSuccess) rc = wc_fail(ctx, WC_ERR_HIP, "wc_map_create: memset");
  if (rc == WC_OK && hipHostMalloc((void **)&m->h_ctr, kCtrWords * 8) != hipSuccess) rc = wc_fail(ctx, WC_ERR_HIP, "wc_map_create: pinned counters");
  if (rc == WC_OK && hipEventCreateWithFlags(&m->ev_ctr, hipEventDisableTiming) != hipSuccess) rc = wc_fail(ctx, WC_ERR_HIP, "wc_map_create: event");
  if (rc != WC_OK) {
    (void)hipGetLastError();
    wc_map_destroy(ctx, m);
    return rc;
  }
  std::memset(m->h_ctr, 0, kCtrWords * 8);
  *out = m;
  return WC_OK;
}

extern "C" int wc_map_destroy(wc_ctx *ctx, wc_map *m) {
  wc_dev_guard dg_(ctx);
  if (!m) return WC_OK;
  if (!map_ok(ctx, m)) return wc_fail(ctx, WC_ERR_ARG, "%s: the map belongs to another context", __func__);
  map_free(ctx, m->keys);
  map_free(ctx, m->pay);
  map_free(ctx, m->mom);
  map_free(ctx, m->ctr);
  for (wc_buf &b : m->b_pairs) wc_buf_release(ctx, b);
  wc_buf_release(ctx, m->b_tmp);
  wc_buf_release(ctx, m->b_cnt);
  wc_buf_release(ctx, m->b_lin);
  wc_buf_release(ctx, m->b_pose);
  wc_buf_release(ctx, m->b_carve);
  wc_buf_release(ctx, m->b_cast);
  wc_buf_release(ctx, m->b_score);
  wc_buf_release(ctx, m->b_ct);
  wc_buf_release(ctx, m->b_cc_idx);
  wc_buf_release(ctx, m->b_cc);
  wc_buf_release(ctx, m->b_cc_comps);
  wc_buf_release(ctx, m->b_cc_tmp);
  (void)hipStreamSynchronize(ctx->stream);  // (the pinned counters may still be the target of an enqueued copy)
  if (m->ev_ctr) (void)hipEventDestroy(m->ev_ctr);
  if (m->h_ctr) (void)hipHostFree(m->h_ctr);
  if (m->h_lin) (void)hipHostFree(m->h_lin);
  if (m->h_pose) (void)hipHostFree(m->h_pose);
  if (m->h_carve) (void)hipHostFree(m->h_carve);
  if (m->h_cast) (void)hipHostFree(m->h_cast);
  if (m->h_score) (void)hipHostFree(m->h_score);
  if (m->h_ct) (void)hipHostFree(m->h_ct);
  if (m->h_cc) (void)hipHostFree(m->h_cc);
  delete m;
  return WC_OK;
}

namespace {
// what precedes every call that may create up to n voxels (insert: n points; absorb: n records; merge: the source's voxels) - growth
// (policy at the top of the file): at most half full at every probe of the call, tombstones counted as full slots.  The decision is
// map_room.h's; a replacement of either kind drops the tombstones (k_map_rehash does not move them)
int map_make_room(wc_ctx *ctx, wc_map *m, uint64_t n, const char *fn) {
  uint64_t cap = 0;
  const int what = map_room(m->cap, map_bound(m), m->tombs, n, &cap);
  if (what == kMapRoomFull) return wc_fail(ctx, WC_ERR_CAPACITY, "%s: the table would exceed 2^32 slots", fn);
  if (what != kMapRoomKeep) {
    WC_TRY(map_replace_table(ctx, m, cap, map_sel_all{}));
    ++(what == kMapRoomGrow ? m->growths : m->purges);
    m->tombs = 0;
  }
  return WC_OK;
}
// ... and what follows its kernel: the n possible new voxels enter the bound; with h_n_rejected the call waits and reports its own
// rejected count, without it the counters travel back behind the kernel and tighten the next call's bound when they have arrived
int map_added(wc_ctx *ctx, wc_map *m, uint64_t n, uint64_t *h_n_rejected) {
  m->pts_since += n;
  if (h_n_rejected) {
    WC_TRY(map_sync_counters(ctx, m));
    *h_n_rejected = m->h_ctr[kCtrRejCall];
    return WC_OK;
  }
  if (m->ctr_pending) {
    m->pts_after_copy += n;
  } else {
    WC_HIP(ctx, hipMemcpyAsync(m->h_ctr, m->ctr, kCtrWords * 8, hipMemcpyDeviceToHost, ctx->stream));
    WC_HIP(ctx, hipEventRecord(m->ev_ctr, ctx->stream));
    m->ctr_pending = true;
    m->pts_after_copy = 0;
  }
  return WC_OK;
}
}  // namespace

extern "C" int wc_map_insert(wc_ctx *ctx, wc_map *m, const wc_points *pts, uint64_t *h_n_rejected) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !map_points_ok(pts)) return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument", __func__);
  if (h_n_rejected) *h_n_rejected = 0;
  if (pts->n == 0) return WC_OK;
  WC_TRY(map_make_room(ctx, m, pts->n, __func__));
  WC_HIP(ctx, hipMemsetAsync(m->ctr + kCtrRejCall, 0, 8, ctx->stream));
  if (!m->mom)
    map_launch_insert<false, kMapPts>(ctx, m, *pts);
  else if (ctx->dev.map_mom_pts == 2)  // (development option: the plain insert's tile, 108 KB of LDS, one workgroup per CU)
    map_launch_insert<true, kMapPts>(ctx, m, *pts);
  else
    map_launch_insert<true, kMapMomPts>(ctx, m, *pts);
  WC_HIP(ctx, hipGetLastError());
  return map_added(ctx, m, pts->n, h_n_rejected);
}

extern "C" int wc_map_size(wc_ctx *ctx, wc_map *m, uint64_t *h_voxels, uint64_t *h_points) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m)) return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument", __func__);
  WC_TRY(map_sync_counters(ctx, m));
  if (h_voxels) *h_voxels = m->h_ctr[kCtrOcc];
  if (h_points) *h_points = m->h_ctr[kCtrPts];
  return WC_OK;
}

extern "C" int wc_map_info(wc_ctx *ctx, wc_map *m, uint64_t h_info[4]) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !h_info) return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument", __func__);
  WC_TRY(map_sync_counters(ctx, m));
  h_info[0] = m->cap;
  h_info[1] = m->growths;
  h_info[2] = m->h_ctr[kCtrRej];
  h_info[3] = m->cap * (m->mom ? 40 + 8 * kMapMom : 40);
  return WC_OK;
}

namespace {
// export, steps 1 and 2: the n occupied slots as (key, slot) pairs in ascending key order, in the map's scratch
int map_sorted_slots(wc_ctx *ctx, wc_map *m, uint64_t n, unsigned long long **skeys, uint32_t **sslots) {
  WC_TRY(wc_ensure(ctx, m->b_pairs[0], n * 8));
  WC_TRY(wc_ensure(ctx, m->b_pairs[1], n * 8));
  WC_TRY(wc_ensure(ctx, m->b_pairs[2], n * 4));
  WC_TRY(wc_ensure(ctx, m->b_pairs[3], n * 4));
  WC_TRY(wc_ensure(ctx, m->b_cnt, 8));
  unsigned long long *kin = (unsigned long long *)m->b_pairs[0].p, *kout = (unsigned long long *)m->b_pairs[1].p;
  uint32_t *vin = (uint32_t *)m->b_pairs[2].p, *vout = (uint32_t *)m->b_pairs[3].p;
  WC_HIP(ctx, hipMemsetAsync(m->b_cnt.p, 0, 8, ctx->stream));
  k_map_compact<<<(unsigned)((m->cap + kCompactChunk - 1) / kCompactChunk), 256, 0, ctx->stream>>>(m->keys, m->cap, kin, vin, n,
                                                                                                   (unsigned long long *)m->b_cnt.p);
  WC_HIP(ctx, hipGetLastError());
  // the slots' order depends on the schedule; the keys are distinct, so the sorted order does not
  using cfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;
  size_t tmp = 0;
  WC_HIP(ctx, rocprim::radix_sort_pairs<cfg>(nullptr, tmp, kin, kout, vin, vout, (size_t)n, 0u, 63u, ctx->stream));
  WC_TRY(wc_ensure(ctx, m->b_tmp, tmp));
  tmp = m->b_tmp.cap;
  WC_HIP(ctx, rocprim::radix_sort_pairs<cfg>(m->b_tmp.p, tmp, kin, kout, vin, vout, (size_t)n, 0u, 63u, ctx->stream));
  *skeys = kout, *sslots = vout;
  return WC_OK;
}
// what both exports begin with: the size read-back into *h_n and the capacity error.  *h_n = 0: an empty map, nothing to write
int map_export_size(wc_ctx *ctx, wc_map *m, const char *fn, uint64_t cap, uint64_t *h_n) {
  WC_TRY(map_sync_counters(ctx, m));
  *h_n = m->h_ctr[kCtrOcc];
  if (cap < *h_n && *h_n)
    return wc_fail(ctx, WC_ERR_CAPACITY, "%s: %llu voxels, capacity %llu", fn, (unsigned long long)*h_n, (unsigned long long)cap);
  return WC_OK;
}
}  // namespace

extern "C" int wc_map_export(wc_ctx *ctx, wc_map *m, float *d_xyz, uint32_t *d_count, int32_t *d_keys, uint64_t cap, uint64_t *h_n) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !h_n) return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument", __func__);
  WC_TRY(map_export_size(ctx, m, __func__, cap, h_n));
  const uint64_t n = *h_n;
  if (n == 0) return WC_OK;
  if (!d_xyz || !d_count) return wc_fail(ctx, WC_ERR_ARG, "%s: null output", __func__);
  unsigned long long *kout = nullptr;
  uint32_t *vout = nullptr;
  WC_TRY(map_sorted_slots(ctx, m, n, &kout, &vout));
  k_map_centroids<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(kout, vout, n, m->pay, m->voxel, d_xyz, d_count, d_keys);
  WC_HIP(ctx, hipGetLastError());
  return WC_OK;
}

extern "C" int wc_map_export_surfels(wc_ctx *ctx, wc_map *m, wc_map_surfel *d_out, uint64_t cap, uint64_t *h_n) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !h_n || !m->mom)
    return wc_fail(ctx, WC_ERR_ARG, "%s: null argument, or a map created without WC_MAP_MOMENTS", __func__);
  WC_TRY(map_export_size(ctx, m, __func__, cap, h_n));
  const uint64_t n = *h_n;
  if (n == 0) return WC_OK;
  if (!d_out || (uintptr_t)d_out % 8) return wc_fail(ctx, WC_ERR_ARG, "%s: null or misaligned output", __func__);
  unsigned long long *kout = nullptr;
  uint32_t *vout = nullptr;
  WC_TRY(map_sorted_slots(ctx, m, n, &kout, &vout));
  k_map_surfels<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(kout, vout, n, m->pay, m->mom, m->voxel, d_out);
  WC_HIP(ctx, hipGetLastError());
  return WC_OK;
}

// ---- the exact state (include/wildcat_hip.h: wc_map_export_state, wc_map_absorb, wc_map_merge) -----------------------------------
extern "C" int wc_map_export_state(wc_ctx *ctx, wc_map *m, wc_map_voxel *d_vox, int64_t *d_mom, uint64_t cap, uint64_t *h_n) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !h_n || (uintptr_t)d_vox % 8 || (uintptr_t)d_mom % 8 || (d_mom && !m->mom))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or misaligned argument, a map of another context, or d_mom with a map created without WC_MAP_MOMENTS",
                   __func__);
  WC_TRY(map_export_size(ctx, m, __func__, cap, h_n));
  const uint64_t n = *h_n;
  if (n == 0) return WC_OK;
  if (!d_vox) return wc_fail(ctx, WC_ERR_ARG, "%s: null output", __func__);
  unsigned long long *kout = nullptr;
  uint32_t *vout = nullptr;
  WC_TRY(map_sorted_slots(ctx, m, n, &kout, &vout));
  k_map_state<<<(unsigned)((n + kStateThreads - 1) / kStateThreads), kStateThreads, 0, ctx->stream>>>(kout, vout, n, m->pay, m->mom, d_vox,
                                                                                                     (long long *)d_mom);
  WC_HIP(ctx, hipGetLastError());
  return WC_OK;
}

extern "C" int wc_map_absorb(wc_ctx *ctx, wc_map *m, const wc_map_voxel *d_vox, const int64_t *d_mom, uint64_t n, uint64_t *h_n_rejected) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m)) return wc_fail(ctx, WC_ERR_ARG, "%s: null argument or a map of another context", __func__);
  if (h_n_rejected) *h_n_rejected = 0;
  if (n == 0) return WC_OK;
  if (!d_vox || (uintptr_t)d_vox % 8 || (uintptr_t)d_mom % 8 || (m->mom && !d_mom) || n > ((uint64_t)1 << 31))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or misaligned records, n > 2^31, or a WC_MAP_MOMENTS map without d_mom", __func__);
  WC_TRY(map_make_room(ctx, m, n, __func__));
  WC_HIP(ctx, hipMemsetAsync(m->ctr + kCtrRejCall, 0, 8, ctx->stream));
  const uint64_t blocks = (n + kStateThreads - 1) / kStateThreads;
  uint64_t grid = std::min<uint64_t>(blocks, (uint64_t)8 * m->cus);
  if (ctx->dev.map_absorb_groups > 0) grid = std::min<uint64_t>(blocks, (uint64_t)ctx->dev.map_absorb_groups);  // (development option)
  if (m->mom)
    k_map_absorb<true><<<(unsigned)grid, kStateThreads, 0, ctx->stream>>>(d_vox, (const long long *)d_mom, n, m->keys, m->pay, m->mom, m->cap - 1,
                                                                          m->ctr);
  else
    k_map_absorb<false><<<(unsigned)grid, kStateThreads, 0, ctx->stream>>>(d_vox, nullptr, n, m->keys, m->pay, nullptr, m->cap - 1, m->ctr);
  WC_HIP(ctx, hipGetLastError());
  return map_added(ctx, m, n, h_n_rejected);
}

extern "C" int wc_map_merge(wc_ctx *ctx, wc_map *dst, wc_map *src) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, dst) || !map_ok(ctx, src) || dst == src || std::memcmp(&dst->voxel, &src->voxel, sizeof(double)) != 0 || (dst->mom && !src->mom))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null argument, dst == src, a map of another context, two voxel sizes, or moments in dst and none in src",
                   __func__);
  WC_TRY(map_sync_counters(ctx, src));  // (the wait: the source's exact voxel count bounds what the destination may gain)
  const uint64_t n = src->h_ctr[kCtrOcc];
  if (n == 0) return WC_OK;
  WC_TRY(map_make_room(ctx, dst, n, __func__));
  const unsigned grid = (unsigned)((src->cap + kStateThreads - 1) / kStateThreads);
  if (dst->mom)
    k_map_merge<true><<<grid, kStateThreads, 0, ctx->stream>>>(src->keys, src->pay, src->mom, src->cap, dst->keys, dst->pay, dst->mom, dst->cap - 1,
                                                               dst->ctr);
  else
    k_map_merge<false><<<grid, kStateThreads, 0, ctx->stream>>>(src->keys, src->pay, nullptr, src->cap, dst->keys, dst->pay, nullptr, dst->cap - 1,
                                                                dst->ctr);
  WC_HIP(ctx, hipGetLastError());
  return map_added(ctx, dst, n, nullptr);
}

// ---- a state under a rigid pose (include/wildcat_hip.h: wc_map_merge_moved, wc_map_move_state) ---------------------
namespace {
// a pose the move accepts: twelve finite entries and |(R^T R - I)_ij| <= 1e-9, (R^T R)_ij = (R_0i R_0j + R_1i R_1j) + R_2i R_2j
bool map_pose_rigid(const double *T) {
  if (!T) return false;
  for (int j = 0; j < 12; ++j)
    if (!std::isfinite(T[j])) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double g = (T[i] * T[j] + T[4 + i] * T[4 + j]) + T[8 + i] * T[8 + j];
      if (!(std::fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-9)) return false;
    }
  return true;
}
}  // namespace

extern "C" int wc_map_merge_moved(wc_ctx *ctx, wc_map *dst, wc_map *src, const double T[12], uint64_t h_out[4]) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, dst) || !map_ok(ctx, src) || dst == src || std::memcmp(&dst->voxel, &src->voxel, sizeof(double)) != 0 ||
      (dst->mom && !src->mom) || !map_pose_rigid(T))
    return wc_fail(ctx, WC_ERR_ARG,
                   "%s: null argument, dst == src, a map of another context, two voxel sizes, moments in dst and none in src, or a T that is "
                   "not finite or not rigid (|R^T R - I| <= 1e-9)",
                   __func__);
  WC_TRY(map_sync_counters(ctx, src));  // (the wait: the source's exact voxel count bounds what the destination may gain)
  const uint64_t n = src->h_ctr[kCtrOcc];
  if (n == 0) {
    if (h_out) h_out[0] = h_out[1] = h_out[2] = h_out[3] = 0;
    return WC_OK;
  }
  WC_TRY(map_make_room(ctx, dst, n, __func__));
  WC_HIP(ctx, hipMemsetAsync(dst->ctr + kCtrMvVox, 0, (size_t)(kCtrMvEnd - kCtrMvVox) * 8, ctx->stream));
  map_pose P;
  std::memcpy(P.T, T, sizeof(P.T));
  const unsigned grid = (unsigned)((src->cap + kStateThreads - 1) / kStateThreads);
  if (dst->mom)
    k_map_merge_moved<true><<<grid, kStateThreads, 0, ctx->stream>>>(src->keys, src->pay, src->mom, src->cap, src->voxel, P, dst->keys, dst->pay,
                                                                     dst->mom, dst->cap - 1, dst->ctr);
  else
    k_map_merge_moved<false><<<grid, kStateThreads, 0, ctx->stream>>>(src->keys, src->pay, nullptr, src->cap, src->voxel, P, dst->keys, dst->pay,
                                                                      nullptr, dst->cap - 1, dst->ctr);
  WC_HIP(ctx, hipGetLastError());
  if (!h_out) return map_added(ctx, dst, n, nullptr);
  dst->pts_since += n;  // (as map_added: the n possible new voxels stay in the bound if the read-back fails)
  WC_TRY(map_sync_counters(ctx, dst));
  h_out[0] = dst->h_ctr[kCtrMvVox], h_out[1] = dst->h_ctr[kCtrMvPts], h_out[2] = dst->h_ctr[kCtrMvRejVox], h_out[3] = dst->h_ctr[kCtrMvRejPts];
  return WC_OK;
}

extern "C" int wc_map_move_state(const wc_map_voxel *vox, const int64_t *mom, uint64_t n, double voxel, const double T[12], wc_map_voxel *out_vox,
                                 int64_t *out_mom, uint64_t *n_rejected) {
  if (!(voxel >= 0.01 && voxel <= 4.0) || !map_pose_rigid(T) || (n && (!vox || !out_vox)) || (mom != nullptr) != (out_mom != nullptr))
    return WC_ERR_ARG;
  double P[12];
  std::memcpy(P, T, sizeof(P));
  uint64_t rej = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const wc_map_voxel &r = vox[i];
    unsigned long long w[kMapMom] = {};
    if (mom)
      for (int j = 0; j < kMapMom; ++j) w[j] = (unsigned long long)mom[kMapMom * i + j];
    bool ok = r.key[0] > -kMapKeyOff && r.key[0] < kMapKeyOff && r.key[1] > -kMapKeyOff && r.key[1] < kMapKeyOff && r.key[2] > -kMapKeyOff &&
              r.key[2] < kMapKeyOff && r.count >= 1u && r.count <= kStateMaxCount;  // (what wc_map_absorb accepts)
    map_moved_voxel o;
    if (ok)
      ok = mom ? map_move_voxel<true>(r.key[0], r.key[1], r.key[2], r.count, r.sum[0], r.sum[1], r.sum[2], w, voxel, P, o)
               : map_move_voxel<false>(r.key[0], r.key[1], r.key[2], r.count, r.sum[0], r.sum[1], r.sum[2], w, voxel, P, o);
    wc_map_voxel q;
    std::memset(&q, 0, sizeof(q));
    if (ok) {
      q.count = r.count;
      for (int a = 0; a < 3; ++a) q.key[a] = o.K[a], q.sum[a] = (int64_t)o.S[a];
    } else {
      ++rej;
    }
    out_vox[i] = q;
    if (mom)
      for (int j = 0; j < kMapMom; ++j) out_mom[kMapMom * i + j] = ok ? (int64_t)o.w[j] : 0;
  }
  if (n_rejected) *n_rejected = rej;
  return WC_OK;
}

// ---- a coarser level(include/wildcat_hip.h: wc_map_coarsen) ----------------------------------------------------------
extern "C" int wc_map_coarsen(wc_ctx *ctx, wc_map *src, uint32_t factor, uint32_t flags, wc_map **out) {
  wc_dev_guard dg_(ctx);
  const bool mom = (flags & WC_MAP_MOMENTS) != 0;
  if (!map_ok(ctx, src) || !out || factor < 1 || !((double)factor * src->voxel <= 4.0) || (flags & ~(uint32_t)WC_MAP_MOMENTS) || (mom && !src->mom))
    return wc_fail(ctx, WC_ERR_ARG,
                   "%s: null argument, a map of another context, factor < 1, factor * voxel > 4.0, unknown flags, or WC_MAP_MOMENTS with a source "
                   "created without it",
                   __func__);
  const double V = (double)factor * src->voxel;  // one fp64 product
  WC_TRY(map_sync_counters(ctx, src));           // (the wait: the source's exact voxel count bounds the result's, its point count is checked)
  const uint64_t n = src->h_ctr[kCtrOcc], limit = (uint64_t)1 << (mom ? 28 : 30);
  if (src->h_ctr[kCtrPts] > limit)
    return wc_fail(ctx, WC_ERR_CAPACITY, "%s: the source holds %llu points, one voxel of the result at most %llu", __func__,
                   (unsigned long long)src->h_ctr[kCtrPts], (unsigned long long)limit);
  wc_map *m = nullptr;
  WC_TRY(wc_map_create_ex(ctx, V, n, flags, &m));  // pow2_at_least(2 n) slots: what wc_map_merge grows an empty destination to
  if (n) {
    const unsigned grid = (unsigned)((src->cap + kStateThreads - 1) / kStateThreads);
    if (mom)
      k_map_coarsen<true><<<grid, kStateThreads, 0, ctx->stream>>>(src->keys, src->pay, src->mom, src->cap, src->voxel, V, (int)factor, m->keys,
                                                                   m->pay, m->mom, m->cap - 1, m->ctr);
    else
      k_map_coarsen<false><<<grid, kStateThreads, 0, ctx->stream>>>(src->keys, src->pay, nullptr, src->cap, src->voxel, V, (int)factor, m->keys,
                                                                    m->pay, nullptr, m->cap - 1, m->ctr);
    int rc = hipGetLastError() == hipSuccess ? WC_OK : wc_fail(ctx, WC_ERR_HIP, "%s: launch", __func__);
    if (rc == WC_OK) rc = map_added(ctx, m, n, nullptr);
    if (rc != WC_OK) {
      wc_map_destroy(ctx, m);
      return rc;
    }
  }
  *out = m;
  return WC_OK;
}

extern "C" int wc_map_clear(wc_ctx *ctx, wc_map *m) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m)) return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument", __func__);
  WC_TRY(map_clear_table(ctx, m->cap, m->keys, m->pay, m->mom));
  WC_HIP(ctx, hipMemsetAsync(m->ctr, 0, kCtrWords * 8, ctx->stream));
  WC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (a pending counter copy lands before the host's bookkeeping is reset)
  m->occ_known = m->pts_since = m->pts_after_copy = 0;
  m->tombs = 0;  // (the empty mark has overwritten them)
  m->ctr_pending = false;
  std::memset(m->h_ctr, 0, kCtrWords * 8);
  return WC_OK;
}

namespace {
// wc_map_nearest (min_points = 0: wc_map_hit records) and wc_map_nearest_plane (min_points >= 3: wc_map_plane_hit records)
int map_nearest(wc_ctx *ctx, wc_map *m, const wc_points *queries, double max_dist, unsigned min_points, void *d_hits, uint64_t *h_n_found,
                const char *fn) {
  wc_dev_guard dg_(ctx);
  const wc_points *q = queries;
  if (!map_ok(ctx, m) || !map_points_ok(q) || !(max_dist > 0.0) || (q->n && (!d_hits || (uintptr_t)d_hits % 8)))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument (max_dist > 0)", fn);
  if (h_n_found) *h_n_found = 0;
  if (q->n == 0) return WC_OK;
  const double max_d2 = max_dist * max_dist;  // (formed once, here: the kernel accepts d2 <= max_d2)
  if (h_n_found) WC_HIP(ctx, hipMemsetAsync(m->ctr + kCtrFound, 0, 8, ctx->stream));
  const uint64_t blocks = (q->n + kNearThreads - 1) / kNearThreads;
  const unsigned grid = (unsigned)std::min<uint64_t>(blocks, (uint64_t)8 * m->cus);
  if (min_points)
    k_map_nearest<true><<<grid, kNearThreads, 0, ctx->stream>>>(*q, m->voxel, max_d2, m->keys, m->pay, m->cap - 1, d_hits, m->ctr + kCtrFound,
                                                                m->mom, min_points);
  else
    k_map_nearest<false><<<grid, kNearThreads, 0, ctx->stream>>>(*q, m->voxel, max_d2, m->keys, m->pay, m->cap - 1, d_hits, m->ctr + kCtrFound,
                                                                 nullptr, 0u);
  WC_HIP(ctx, hipGetLastError());
  if (h_n_found) {
    WC_HIP(ctx, hipMemcpyAsync(m->h_ctr + kCtrFound, m->ctr + kCtrFound, 8, hipMemcpyDeviceToHost, ctx->stream));
    WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *h_n_found = m->h_ctr[kCtrFound];
  }
  return WC_OK;
}
}  // namespace

extern "C" int wc_map_nearest(wc_ctx *ctx, wc_map *m, const wc_points *queries, double max_dist, wc_map_hit *d_hits, uint64_t *h_n_found) {
  return map_nearest(ctx, m, queries, max_dist, 0u, d_hits, h_n_found, __func__);
}

extern "C" int wc_map_nearest_plane(wc_ctx *ctx, wc_map *m, const wc_points *queries, double max_dist, uint32_t min_points,
                                    wc_map_plane_hit *d_hits, uint64_t *h_n_found) {
  if (map_ok(ctx, m) && (!m->mom || min_points < 3)) {
    wc_dev_guard dg_(ctx);
    return wc_fail(ctx, WC_ERR_ARG, "%s: a map created without WC_MAP_MOMENTS, or min_points < 3", __func__);
  }
  return map_nearest(ctx, m, queries, max_dist, min_points, d_hits, h_n_found, __func__);
}

namespace {
template <int KMAX, int REACH>
void knn_launch(wc_ctx *ctx, wc_map *m, const wc_points &q, double max_d2, const wc_map_knn_params &p, wc_map_hit *d_hits, uint32_t *d_within,
                unsigned grid) {
  k_map_knn<KMAX, REACH><<<grid, kKnnThreads, 0, ctx->stream>>>(q, m->voxel, max_d2, p.k, p.min_points, p.flags & WC_MAP_KNN_NOT_OWN, m->keys,
                                                                m->pay, m->cap - 1, d_hits, d_within, m->ctr + kCtrKnnSome,
                                                                m->ctr + kCtrKnnRec, m->ctr + kCtrKnnWithin);
}
template <int REACH>
void knn_launch_k(wc_ctx *ctx, wc_map *m, const wc_points &q, double max_d2, const wc_map_knn_params &p, wc_map_hit *d_hits, uint32_t *d_within,
                  unsigned grid) {
  // the smallest instantiation that holds k entries
  if (p.k <= 1) knn_launch<1, REACH>(ctx, m, q, max_d2, p, d_hits, d_within, grid);
  else if (p.k <= 4) knn_launch<4, REACH>(ctx, m, q, max_d2, p, d_hits, d_within, grid);
  else if (p.k <= 8) knn_launch<8, REACH>(ctx, m, q, max_d2, p, d_hits, d_within, grid);
  else knn_launch<16, REACH>(ctx, m, q, max_d2, p, d_hits, d_within, grid);
}
}  // namespace

extern "C" int wc_map_knn(wc_ctx *ctx, wc_map *m, const wc_points *queries, const wc_map_knn_params *params, wc_map_hit *d_hits,
                          uint32_t *d_within, uint64_t h_out[3]) {
  wc_dev_guard dg_(ctx);
  const wc_points *q = queries;
  const wc_map_knn_params *p = params;
  if (!map_ok(ctx, m) || !map_points_ok(q) || !p || !(p->max_dist > 0.0) || p->k < 1 || p->k > 16 || (p->reach != 1 && p->reach != 2) ||
      p->min_points < 1 || (p->flags & ~(uint32_t)WC_MAP_KNN_NOT_OWN) || (q->n && (!d_hits || (uintptr_t)d_hits % 8)) ||
      (uintptr_t)d_within % 4)
    return wc_fail(ctx, WC_ERR_ARG,
                   "%s: null or out-of-range argument (max_dist > 0, k in 1 .. 16, reach 1 or 2, min_points >= 1, known flags, a map of "
                   "this context)",
                   __func__);
  if (h_out) h_out[0] = h_out[1] = h_out[2] = 0;
  if (q->n == 0) return WC_OK;
  const double max_d2 = p->max_dist * p->max_dist;  // (formed once, here: the kernel accepts d2 <= max_d2)
  if (h_out) WC_HIP(ctx, hipMemsetAsync(m->ctr + kCtrKnnSome, 0, (size_t)(kCtrWords - kCtrKnnSome) * 8, ctx->stream));
  const uint64_t blocks = (q->n + kKnnThreads - 1) / kKnnThreads;
  const unsigned grid = (unsigned)std::min<uint64_t>(blocks, (uint64_t)8 * m->cus);
  if (p->reach == 1)
    knn_launch_k<1>(ctx, m, *q, max_d2, *p, d_hits, d_within, grid);
  else
    knn_launch_k<2>(ctx, m, *q, max_d2, *p, d_hits, d_within, grid);
  WC_HIP(ctx, hipGetLastError());
  if (h_out) {
    WC_HIP(ctx, hipMemcpyAsync(m->h_ctr + kCtrKnnSome, m->ctr + kCtrKnnSome, (size_t)(kCtrWords - kCtrKnnSome) * 8, hipMemcpyDeviceToHost,
                               ctx->stream));
    WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h_out[0] = m->h_ctr[kCtrKnnSome], h_out[1] = m->h_ctr[kCtrKnnRec], h_out[2] = m->h_ctr[kCtrKnnWithin];
  }
  return WC_OK;
}

// ---- registration against the map (include/wildcat_hip.h: wc_map_linearize, wc_map_align) ------------------------------------------
namespace {
bool reg_params_ok(const wc_map_reg_params *p) {
  return p && p->max_dist > 0.0 && p->min_points >= 3 && p->reserved == 0 && p->sigma0 > 0.0 && std::isfinite(p->sigma0) &&
         p->cauchy_a >= 0.0 && std::isfinite(p->cauchy_a);
}
// the sizes of the reduction's levels: m_0 = tiles, m_(l+1) = ceil(m_l / 32) down to 1 (at least one level: a copy when tiles = 1)
uint64_t lin_words(uint64_t tiles) {
  uint64_t total = tiles, m = tiles;
  do {
    m = (m + kLinFan - 1) / kLinFan;
    total += m;
  } while (m > 1);
  return total * kLinWords;
}
map_reg reg_of(const wc_map_reg_params *params) {
  map_reg R;
  R.max_d2 = params->max_dist * params->max_dist;
  R.s02 = params->sigma0 * params->sigma0;
  R.a2 = params->cauchy_a * params->cauchy_a;
  R.min_points = params->min_points;
  return R;
}
// a final partial (28 doubles, then n_used, n_found, n_bad) as the record
void normal_eq_of(const unsigned long long *part, wc_map_normal_eq *out) {
  double sums[kLinSums];
  std::memcpy(sums, part, sizeof(sums));
  for (int e = 0; e < 21; ++e) out->H[e] = sums[e];
  for (int e = 0; e < 6; ++e) out->g[e] = sums[21 + e];
  out->cost = 0.5 * sums[27];
  out->n_used = part[kLinSums], out->n_found = part[kLinSums + 1];
}
// what every registration call asks of its map, points and params: a map of this context with moments, readable points, valid params
bool reg_args_ok(const wc_ctx *ctx, const wc_map *m, const wc_points *pts, const wc_map_reg_params *params) {
  return map_ok(ctx, m) && m->mom && map_points_ok(pts) && reg_params_ok(params);
}
// K poses (K x 12 doubles) without a non-finite entry: the registration's and the score's check
int poses_finite(wc_ctx *ctx, const double *T, uint32_t K, const char *fn) {
  for (uint64_t j = 0; j < (uint64_t)K * 12; ++j)
    if (!std::isfinite(T[j]))
      return wc_fail(ctx, WC_ERR_ARG, "%s: entry %u of hypothesis %u's T is not finite", fn, (unsigned)(j % 12), (unsigned)(j / 12));
  return WC_OK;
}
constexpr uint32_t kLinBatchMax = 1024;         // hypotheses of one call
constexpr uint64_t kLinBatchItems = 1ull << 20;  // (hypothesis, tile) pairs of one batched call: a design cap, about 270 MB of partials
// The linearisation at K >= 1 poses behind the entry points' argument checks: every hypothesis's record and status (WC_OK, or WC_ERR_ARG
// and a zero record where the pose sends a finite point to a non-finite one).  One launch of k_map_linearize, one of k_map_lin_reduce per
// level, one copy of K x 256 bytes, one wait.  K = 1: the pose travels in the kernel arguments (no copy to the device) and rows may be
// non-null; K > 1: the poses are uploaded from their pinned block first
int lin_core(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double *T, uint32_t K, const wc_map_reg_params *params, wc_map_reg_row *rows,
             wc_map_normal_eq *h_out, int32_t *h_status) {
  std::memset(h_out, 0, (size_t)K * sizeof(*h_out));
  for (uint32_t h = 0; h < K; ++h) h_status[h] = WC_OK;
  if (pts->n == 0) return WC_OK;
  const uint64_t tiles = (pts->n + kLinThreads - 1) / kLinThreads, hyp_words = lin_words(tiles);
  // the partials hypothesis-major, then the K final partials side by side (the last level writes there, not into its own slot)
  WC_TRY(wc_ensure(ctx, m->b_lin, ((uint64_t)K * hyp_words + (uint64_t)K * kLinWords) * 8));
  if (m->h_lin_cap < K) {
    if (m->h_lin) (void)hipHostFree(m->h_lin);
    if (m->h_pose) (void)hipHostFree(m->h_pose);
    m->h_lin = nullptr, m->h_pose = nullptr, m->h_lin_cap = 0;
    WC_HIP(ctx, hipHostMalloc((void **)&m->h_lin, (size_t)K * kLinWords * 8));
    if (K > 1) WC_HIP(ctx, hipHostMalloc((void **)&m->h_pose, (size_t)K * 12 * sizeof(double)));
    m->h_lin_cap = K;
  }
  unsigned long long *base = (unsigned long long *)m->b_lin.p, *fin = base + (uint64_t)K * hyp_words;
  const map_reg R = reg_of(params);
  const uint64_t items = (uint64_t)K * tiles;
  uint64_t grid = std::min<uint64_t>(items, (uint64_t)8 * m->cus);
  if (ctx->dev.map_lin_groups > 0) grid = std::min<uint64_t>(items, (uint64_t)ctx->dev.map_lin_groups);  // (development option)
  if (K == 1) {
    map_pose P;
    std::memcpy(P.T, T, sizeof(P.T));
    k_map_linearize<true><<<(unsigned)grid, kLinThreads, 0, ctx->stream>>>(*pts, P, nullptr, 1u, R, m->voxel, m->keys, m->pay, m->mom, m->cap - 1,
                                                                          rows, base, hyp_words);
  } else {
    WC_TRY(wc_ensure(ctx, m->b_pose, (size_t)K * 12 * sizeof(double)));
    std::memcpy(m->h_pose, T, (size_t)K * 12 * sizeof(double));
    WC_HIP(ctx, hipMemcpyAsync(m->b_pose.p, m->h_pose, (size_t)K * 12 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    k_map_linearize<false><<<(unsigned)grid, kLinThreads, 0, ctx->stream>>>(*pts, map_pose{}, (const double *)m->b_pose.p, K, R, m->voxel, m->keys,
                                                                           m->pay, m->mom, m->cap - 1, nullptr, base, hyp_words);
  }
  WC_HIP(ctx, hipGetLastError());
  uint64_t cnt = tiles, off = 0;  // the level's partials and where they start within a hypothesis
  do {
    const uint64_t nxt = (cnt + kLinFan - 1) / kLinFan, off_out = off + cnt * kLinWords;
    unsigned long long *out = nxt > 1 ? base + off_out : fin;
    const uint64_t out_stride = nxt > 1 ? hyp_words : (uint64_t)kLinWords, lanes = (uint64_t)K * nxt * kLinWords;
    k_map_lin_reduce<kLinWords, kLinSums><<<(unsigned)((lanes + 255) / 256), 256, 0, ctx->stream>>>(base + off, hyp_words, cnt, out, out_stride, K);
    WC_HIP(ctx, hipGetLastError());
    off = off_out, cnt = nxt;
  } while (cnt > 1);
  WC_HIP(ctx, hipMemcpyAsync(m->h_lin, fin, (size_t)K * kLinWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t h = 0; h < K; ++h) {
    const unsigned long long *part = m->h_lin + (size_t)h * kLinWords;
    if (part[kLinSums + 2])
      h_status[h] = WC_ERR_ARG;
    else
      normal_eq_of(part, &h_out[h]);
  }
  return WC_OK;
}
// the single calls' error for a status lin_core left at K = 1 (the count is still in its landing place)
int lin_one_failed(wc_ctx *ctx, const wc_map *m, const char *fn) {
  return wc_fail(ctx, WC_ERR_ARG, "%s: T sends %llu finite points to a non-finite one", fn, m->h_lin[kLinSums + 2]);
}
// what wc_map_linearize_batch refuses of its arguments other than the records it writes; WC_OK: the call may run
int lin_batch_check(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double *T, uint32_t K, const wc_map_reg_params *params, const char *fn) {
  if (!reg_args_ok(ctx, m, pts, params) || (K && !T) || K > kLinBatchMax)
    return wc_fail(ctx, WC_ERR_ARG,
                   "%s: null or out-of-range argument (K <= 1024), a map of another context or one created without WC_MAP_MOMENTS", fn);
  WC_TRY(poses_finite(ctx, T, K, fn));
  if ((uint64_t)K * ((pts->n + kLinThreads - 1) / kLinThreads) > kLinBatchItems)
    return wc_fail(ctx, WC_ERR_CAPACITY, "%s: K * ceil(n / 256) exceeds 2^20", fn);
  return WC_OK;
}
}  // namespace

extern "C" int wc_map_linearize(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double T[12], const wc_map_reg_params *params,
                                wc_map_normal_eq *h_out, wc_map_reg_row *d_rows) {
  wc_dev_guard dg_(ctx);
  if (!reg_args_ok(ctx, m, pts, params) || !T || !h_out || (uintptr_t)d_rows % 8)
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument, a map of another context or one created without WC_MAP_MOMENTS", __func__);
  WC_TRY(poses_finite(ctx, T, 1, __func__));
  int32_t status;
  WC_TRY(lin_core(ctx, m, pts, T, 1, params, d_rows, h_out, &status));
  return status == WC_OK ? WC_OK : lin_one_failed(ctx, m, __func__);
}

extern "C" int wc_map_linearize_batch(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double *T, uint32_t K, const wc_map_reg_params *params,
                                      wc_map_normal_eq *h_out, int32_t *h_status) {
  wc_dev_guard dg_(ctx);
  if (K && (!h_out || !h_status)) return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument", __func__);
  WC_TRY(lin_batch_check(ctx, m, pts, T, K, params, __func__));
  if (K == 0) return WC_OK;
  return lin_core(ctx, m, pts, T, K, params, nullptr, h_out, h_status);
}

namespace {
// Rod(w) = I + A K + B K^2, K = [w]x, A = sin(th) / th, B = (sin(th/2) / (th/2))^2 / 2: the rigid and the continuous-time update's one copy
void rod_matrix(const double w[3], double E[3][3]) {
  const double wx = w[0], wy = w[1], wz = w[2];
  const double th = std::sqrt((wx * wx + wy * wy) + wz * wz);
  double A = 1.0, B = 0.5;
  if (th > 0.0) {
    const double h = std::sin(0.5 * th) / (0.5 * th);
    A = std::sin(th) / th, B = 0.5 * (h * h);
  }
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double k2 = (K[r][0] * K[0][c] + K[r][1] * K[1][c]) + K[r][2] * K[2][c];
      E[r][c] = ((r == c ? 1.0 : 0.0) + A * K[r][c]) + B * k2;
    }
}
// R <- Rod(omega) R, t <- Rod(omega) t + upsilon
void pose_update(double T[12], const double xi[6]) {
  double E[3][3];
  rod_matrix(xi, E);
  double N[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) N[4 * r + c] = ((E[r][0] * T[c] + E[r][1] * T[4 + c]) + E[r][2] * T[8 + c]) + (c == 3 ? xi[3 + r] : 0.0);
  std::memcpy(T, N, sizeof(N));
}
// A xi = -g for the symmetric n x n matrix A (row-major, n <= 12: 6 the rigid registration's, 12 the continuous-time one's) by a Cholesky
// factorisation of A scaled to unit diagonal; false: a pivot (the number under the square root) is not finite or below min_pivot
constexpr int kGnMax = 12;
bool gn_solve(int n, const double *A, const double *g, double min_pivot, double *xi) {
  double D[kGnMax], L[kGnMax][kGnMax] = {}, y[kGnMax];
  for (int a = 0; a < n; ++a) D[a] = 1.0 / std::sqrt(A[a * n + a]);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = (D[i] * A[i * n + j]) * D[j];
      if (i == j) s = 1.0;
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (!std::isfinite(s) || !std::isfinite(D[i]) || !(s >= min_pivot)) return false;
        L[i][i] = std::sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  for (int i = 0; i < n; ++i) {
    double s = -(D[i] * g[i]);
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < n; ++k) s -= L[k][i] * xi[k];
    xi[i] = s / L[i][i];
  }
  for (int i = 0; i < n; ++i) {
    xi[i] *= D[i];
    if (!std::isfinite(xi[i])) return false;
  }
  return true;
}
// the 21 entries of an upper triangle, row-major, into the 6 x 6 block of the n x n matrix A at (r0, c0) - and mirrored, into (c0, r0)
void put_block(const double H[21], int n, double *A, int r0, int c0) {
  for (int a = 0, e = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b, ++e) A[(r0 + a) * n + (c0 + b)] = A[(r0 + b) * n + (c0 + a)] = A[(c0 + b) * n + (r0 + a)] = A[(c0 + a) * n + (r0 + b)] = H[e];
}
bool gn_step(const wc_map_normal_eq &ne, double min_pivot, double xi[6]) {
  double A[36];
  put_block(ne.H, 6, A, 0, 0);
  return gn_solve(6, A, ne.g, min_pivot, xi);
}
bool align_opts_ok(const wc_map_align_opts *o) {
  return o && o->max_iterations >= 1 && o->tol_rot > 0.0 && o->tol_trans > 0.0 && o->min_used >= 6 && o->min_pivot > 0.0;
}
// the Gauss-Newton loop of one start in pieces: the lockstep rounds of align_batch_core call them per hypothesis
enum { kAlignGo = 0, kAlignEndFresh = 1, kAlignEndStale = 2 };  // iterate again; ended, ne is the linearisation at T_io; ended, it is not
void align_begin(wc_map_align_summary *s) {
  std::memset(s, 0, sizeof(*s));
  s->termination = 1;
}
// iteration `it` behind its linearisation ne at T_io
int align_iter(const wc_map_normal_eq &ne, uint32_t it, double T_io[12], const wc_map_align_opts *o, wc_map_align_summary *s) {
  if (it == 0) s->initial_cost = ne.cost;
  double xi[6];
  if (ne.n_used < o->min_used || !gn_step(ne, o->min_pivot, xi)) {
    s->termination = 2;
    return kAlignEndFresh;
  }
  double T[12];
  std::memcpy(T, T_io, sizeof(T));
  pose_update(T, xi);
  bool finite = true;
  for (int j = 0; j < 12; ++j) finite = finite && std::isfinite(T[j]);
  if (!finite) {
    s->termination = 2;
    return kAlignEndFresh;
  }
  std::memcpy(T_io, T, sizeof(T));
  std::memcpy(s->last_step, xi, sizeof(xi));
  s->iterations = (int32_t)(it + 1);
  const double rot = std::sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]), tr = std::sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
  if (rot <= o->tol_rot && tr <= o->tol_trans) {
    s->termination = 0;
    return kAlignEndStale;
  }
  return it + 1 < o->max_iterations ? kAlignGo : kAlignEndStale;
}
// ne: the linearisation at the final T_io
void align_end(const wc_map_normal_eq &ne, wc_map_align_summary *s) {
  s->final_cost = ne.cost;
  s->n_used = ne.n_used, s->n_found = ne.n_found;
}
}  // namespace

namespace {
// The alignment of K >= 1 starts behind the entry points' argument checks.  resume: the hypotheses whose h_status is not WC_OK on entry
// are skipped - T and status stay, the summary is zero (wc_map_align_pyramid_batch's later levels); otherwise every status starts as
// WC_OK.  Round r: ONE lin_core over the compacted poses of the hypotheses that iterate (r < max_iterations) and of those that ended in
// round r - 1 and wait for the linearisation at their final T: at most max_iterations + 1 rounds.  A hypothesis whose linearisation
// fails ends there: its status is the error, its T and summary stay as they stand
int align_batch_core(wc_ctx *ctx, wc_map *m, const wc_points *pts, double *T_io, uint32_t K, const wc_map_align_opts *o, wc_map_align_summary *h_out,
                     int32_t *h_status, bool resume) {
  constexpr int kDone = 3;
  std::vector<int> state(K, kAlignGo);
  for (uint32_t h = 0; h < K; ++h) {
    if (resume && h_status[h] != WC_OK) {
      std::memset(&h_out[h], 0, sizeof(h_out[h]));
      state[h] = kDone;
      continue;
    }
    h_status[h] = WC_OK;
    align_begin(&h_out[h]);
  }
  std::vector<uint32_t> idx;
  std::vector<double> Tc;
  std::vector<wc_map_normal_eq> ne(K);  // (sized once: a round fills a prefix)
  std::vector<int32_t> st(K);
  idx.reserve(K), Tc.reserve((size_t)K * 12);
  for (uint32_t it = 0;; ++it) {
    idx.clear(), Tc.clear();
    for (uint32_t h = 0; h < K; ++h)
      if (state[h] != kDone) {
        idx.push_back(h);
        Tc.insert(Tc.end(), T_io + 12 * (size_t)h, T_io + 12 * (size_t)h + 12);
      }
    if (idx.empty()) break;
    WC_TRY(lin_core(ctx, m, pts, Tc.data(), (uint32_t)idx.size(), &o->reg, nullptr, ne.data(), st.data()));
    for (size_t a = 0; a < idx.size(); ++a) {
      const uint32_t h = idx[a];
      if (st[a] != WC_OK) {
        h_status[h] = st[a], state[h] = kDone;
        continue;
      }
      // (a hypothesis that ended in the round before: this is the linearisation at its final T)
      state[h] = state[h] == kAlignGo ? align_iter(ne[a], it, T_io + 12 * (size_t)h, o, &h_out[h]) : kAlignEndFresh;
      if (state[h] == kAlignEndFresh) {
        align_end(ne[a], &h_out[h]);
        state[h] = kDone;
      }
    }
  }
  return WC_OK;
}
// one start through align_batch_core, its status as the call's error: wc_map_align and a level of wc_map_align_pyramid behind their checks
int align_one(wc_ctx *ctx, wc_map *m, const wc_points *pts, double T_io[12], const wc_map_align_opts *o, wc_map_align_summary *h_out,
              const char *fn) {
  int32_t status;
  WC_TRY(align_batch_core(ctx, m, pts, T_io, 1, o, h_out, &status, false));
  return status == WC_OK ? WC_OK : lin_one_failed(ctx, m, fn);
}
constexpr const char *kAlignOptsMsg =
    "%s: null or out-of-range argument (max_iterations >= 1, tol_rot, tol_trans, min_pivot > 0, min_used >= 6)";
}  // namespace

extern "C" int wc_map_align(wc_ctx *ctx, wc_map *m, const wc_points *pts, double T_io[12], const wc_map_align_opts *o,
                            wc_map_align_summary *h_out) {
  wc_dev_guard dg_(ctx);
  if (!ctx || !T_io || !h_out || !align_opts_ok(o)) return wc_fail(ctx, WC_ERR_ARG, kAlignOptsMsg, __func__);
  align_begin(h_out);  // (a refusal below leaves the summary begun, as it always has)
  if (!reg_args_ok(ctx, m, pts, &o->reg))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument, a map of another context or one created without WC_MAP_MOMENTS", __func__);
  WC_TRY(poses_finite(ctx, T_io, 1, __func__));
  return align_one(ctx, m, pts, T_io, o, h_out, __func__);
}

extern "C" int wc_map_align_batch(wc_ctx *ctx, wc_map *m, const wc_points *pts, double *T_io, uint32_t K, const wc_map_align_opts *o,
                                  wc_map_align_summary *h_out, int32_t *h_status) {
  wc_dev_guard dg_(ctx);
  if (!ctx || (K && (!T_io || !h_out || !h_status)) || !align_opts_ok(o)) return wc_fail(ctx, WC_ERR_ARG, kAlignOptsMsg, __func__);
  WC_TRY(lin_batch_check(ctx, m, pts, T_io, K, &o->reg, __func__));
  if (K == 0) return WC_OK;
  return align_batch_core(ctx, m, pts, T_io, K, o, h_out, h_status, false);
}

// coarse to fine: one start per level, each from the pose the level before it left; the first level whose linearisation fails is the
// call's error, and the later levels' summaries stay untouched.  Everything wc_map_align refuses from its arguments alone is checked for
// every level before the first one runs
extern "C" int wc_map_align_pyramid(wc_ctx *ctx, wc_map *const *levels, uint32_t n_levels, const wc_points *pts, double T_io[12],
                                    const wc_map_align_opts *opts, wc_map_align_summary *h_out) {
  wc_dev_guard dg_(ctx);
  bool ok = ctx && levels && n_levels >= 1 && n_levels <= 8 && T_io && opts && h_out;
  for (int j = 0; ok && j < 12; ++j) ok = std::isfinite(T_io[j]);
  for (uint32_t l = 0; ok && l < n_levels; ++l) ok = reg_args_ok(ctx, levels[l], pts, &opts[l].reg) && align_opts_ok(&opts[l]);
  if (!ok)
    return wc_fail(ctx, WC_ERR_ARG,
                   "%s: null or out-of-range argument (1 <= n_levels <= 8; per level what wc_map_align refuses: a map of another context or one "
                   "created without WC_MAP_MOMENTS, its options), or a T_io that is not finite",
                   __func__);
  for (uint32_t l = 0; l < n_levels; ++l) WC_TRY(align_one(ctx, levels[l], pts, T_io, &opts[l], &h_out[l], __func__));
  return WC_OK;
}

// K hypotheses coarse to fine: level l is one align_batch_core over the hypotheses whose status is still WC_OK
extern "C" int wc_map_align_pyramid_batch(wc_ctx *ctx, wc_map *const *levels, uint32_t n_levels, const wc_points *pts, double *T_io, uint32_t K,
                                          const wc_map_align_opts *opts, wc_map_align_summary *h_out, int32_t *h_status) {
  wc_dev_guard dg_(ctx);
  bool ok = ctx && levels && n_levels >= 1 && n_levels <= 8 && opts && !(K && (!T_io || !h_out || !h_status));
  for (uint32_t l = 0; ok && l < n_levels; ++l) ok = align_opts_ok(&opts[l]);
  if (!ok)
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument (1 <= n_levels <= 8; per level what wc_map_align_batch refuses)", __func__);
  for (uint32_t l = 0; l < n_levels; ++l) WC_TRY(lin_batch_check(ctx, levels[l], pts, T_io, K, &opts[l].reg, __func__));
  for (uint32_t l = 0; l < n_levels && K; ++l)
    WC_TRY(align_batch_core(ctx, levels[l], pts, T_io, K, &opts[l], h_out + (size_t)l * K, h_status, l > 0));
  return WC_OK;
}

// ---- registration of a stamped sweep in continuous time (include/wildcat_hip.h: wc_map_linearize_ct, wc_map_align_ct) -----------------
namespace {
// the two poses and the stamp bounds as the kernel and wc_pose_interp_move take them: span formed once, the end quaternion on the begin
// one's side.  false: a non-finite entry, a quaternion whose squared norm is 0 or not finite, t_end <= t_begin, a non-finite bound or span
bool ct_pose_of(const wc_pose *b, const wc_pose *e, double t_begin, double t_end, map_ct_pose *C) {
  if (!b || !e || !std::isfinite(t_begin) || !std::isfinite(t_end) || !(t_end > t_begin)) return false;
  for (int j = 0; j < 3; ++j) C->p0[j] = b->pos[j], C->p1[j] = e->pos[j];
  for (int j = 0; j < 4; ++j) C->q0[j] = b->quat[j], C->q1[j] = e->quat[j];
  for (int j = 0; j < 3; ++j)
    if (!std::isfinite(C->p0[j]) || !std::isfinite(C->p1[j])) return false;
  for (const double *q : {C->q0, C->q1}) {
    const double nn = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (!std::isfinite(nn) || !(nn > 0.0)) return false;  // (a non-finite entry makes nn non-finite)
  }
  const double dot = ((C->q0[0] * C->q1[0] + C->q0[1] * C->q1[1]) + C->q0[2] * C->q1[2]) + C->q0[3] * C->q1[3];
  if (dot < 0.0)
    for (int j = 0; j < 4; ++j) C->q1[j] = -C->q1[j];
  C->t_begin = t_begin, C->t_end = t_end, C->span = t_end - t_begin;
  return std::isfinite(C->span) && C->span > 0.0;
}
constexpr uint32_t kCtNaN = 0x7fc00000u;  // the quiet NaN of a point out of span in d_xyz_out
// the sizes of the reduction's levels, as lin_words, in partials of kCtWords words
uint64_t ct_words(uint64_t tiles) { return lin_words(tiles) / kLinWords * kCtWords; }
// a final partial (76 doubles, then n_used, n_found, n_outside, n_bad) as the record
void ct_normal_eq_of(const unsigned long long *part, wc_map_ct_normal_eq *out) {
  double sums[kCtSums];
  std::memcpy(sums, part, sizeof(sums));
  for (int e = 0; e < 21; ++e) out->H00[e] = sums[e], out->H01[e] = sums[21 + e], out->H11[e] = sums[42 + e];
  for (int e = 0; e < 6; ++e) out->g0[e] = sums[63 + e], out->g1[e] = sums[69 + e];
  out->cost = 0.5 * sums[75];
  out->n_used = part[kCtSums], out->n_found = part[kCtSums + 1], out->n_outside = part[kCtSums + 2], out->reserved = 0;
}
bool ct_args_ok(const wc_ctx *ctx, const wc_map *m, const wc_points *pts, const wc_map_reg_params *params) {
  return reg_args_ok(ctx, m, pts, params) &&
         (pts->n == 0 || (pts->time && pts->time_stride >= 8 && pts->time_stride % 8 == 0 && (uintptr_t)pts->time % 8 == 0));
}
constexpr const char *kCtArgsMsg =
    "%s: null or out-of-range argument (stamps: 8-aligned doubles; poses: finite, non-zero quaternions; t_begin < t_end, finite), a map of "
    "another context or one created without WC_MAP_MOMENTS";
// The linearisation behind the entry points' checks: one launch of k_map_linearize_ct, one of k_map_lin_reduce<80, 76> per level, one copy
// of 640 bytes, one wait.  *h_out: the record, or zero and WC_ERR_ARG where the poses send a finite point to a non-finite one
int ct_lin_core(wc_ctx *ctx, wc_map *m, const wc_points *pts, const map_ct_pose &C, const wc_map_reg_params *params, wc_map_ct_normal_eq *h_out,
                wc_map_ct_row *d_rows, float *d_xyz_out, const char *fn) {
  std::memset(h_out, 0, sizeof(*h_out));
  if (pts->n == 0) return WC_OK;
  const uint64_t tiles = (pts->n + kLinThreads - 1) / kLinThreads, words = ct_words(tiles);
  WC_TRY(wc_ensure(ctx, m->b_ct, (words + kCtWords) * 8));
  if (!m->h_ct) WC_HIP(ctx, hipHostMalloc((void **)&m->h_ct, (size_t)kCtWords * 8));
  unsigned long long *base = (unsigned long long *)m->b_ct.p, *fin = base + words;
  uint64_t grid = std::min<uint64_t>(tiles, (uint64_t)8 * m->cus);
  if (ctx->dev.map_lin_groups > 0) grid = std::min<uint64_t>(tiles, (uint64_t)ctx->dev.map_lin_groups);  // (development option)
  k_map_linearize_ct<<<(unsigned)grid, kLinThreads, 0, ctx->stream>>>(*pts, C, reg_of(params), m->voxel, m->keys, m->pay, m->mom, m->cap - 1,
                                                                      d_rows, d_xyz_out, base);
  WC_HIP(ctx, hipGetLastError());
  uint64_t cnt = tiles, off = 0;  // the level's partials and where they start
  do {
    const uint64_t nxt = (cnt + kLinFan - 1) / kLinFan, off_out = off + cnt * kCtWords;
    unsigned long long *out = nxt > 1 ? base + off_out : fin;
    const uint64_t lanes = nxt * kCtWords;
    k_map_lin_reduce<kCtWords, kCtSums><<<(unsigned)((lanes + 255) / 256), 256, 0, ctx->stream>>>(base + off, 0, cnt, out, 0, 1u);
    WC_HIP(ctx, hipGetLastError());
    off = off_out, cnt = nxt;
  } while (cnt > 1);
  WC_HIP(ctx, hipMemcpyAsync(m->h_ct, fin, (size_t)kCtWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (m->h_ct[kCtSums + 3])
    return wc_fail(ctx, WC_ERR_ARG, "%s: the poses send %llu finite points to a non-finite one", fn, m->h_ct[kCtSums + 3]);
  ct_normal_eq_of(m->h_ct, h_out);
  return WC_OK;
}
bool ct_prior_ok(const double prior[4]) {
  for (int j = 0; j < 4; ++j)
    if (!(prior[j] >= 0.0) || !std::isfinite(prior[j])) return false;
  return true;
}
// the 12 x 12 step: A = (H00 H01; H01 H11) + diag(w), b = (g0, g1) + w acc
bool ct_step(const wc_map_ct_normal_eq &ne, const double prior[4], const double acc[12], double min_pivot, double xi[12]) {
  double A[144], b[12];
  put_block(ne.H00, 12, A, 0, 0);
  put_block(ne.H11, 12, A, 6, 6);
  put_block(ne.H01, 12, A, 0, 6);
  for (int i = 0; i < 12; ++i) {
    const double w = prior[i / 3];
    A[i * 12 + i] += w;
    b[i] = (i < 6 ? ne.g0[i] : ne.g1[i - 6]) + w * acc[i];
  }
  return gn_solve(12, A, b, min_pivot, xi);
}
// quat <- quat(Rod(omega)) * quat divided by its norm, pos <- Rod(omega) pos + upsilon
void ct_pose_update(wc_pose *P, const double xi[6]) {
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double th = std::sqrt((wx * wx + wy * wy) + wz * wz);
  const double h = th > 0.0 ? std::sin(0.5 * th) / th : 0.5;
  const double dw = std::cos(0.5 * th), dx = h * wx, dy = h * wy, dz = h * wz;
  const double *q = P->quat;
  double r[4];
  r[0] = ((dw * q[0] - dx * q[1]) - dy * q[2]) - dz * q[3];
  r[1] = ((dw * q[1] + dx * q[0]) + dy * q[3]) - dz * q[2];
  r[2] = ((dw * q[2] - dx * q[3]) + dy * q[0]) + dz * q[1];
  r[3] = ((dw * q[3] + dx * q[2]) - dy * q[1]) + dz * q[0];
  const double nrm = std::sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
  for (int j = 0; j < 4; ++j) P->quat[j] = r[j] / nrm;
  double E[3][3];
  rod_matrix(xi, E);
  double t[3];
  for (int a = 0; a < 3; ++a) t[a] = ((E[a][0] * P->pos[0] + E[a][1] * P->pos[1]) + E[a][2] * P->pos[2]) + xi[3 + a];
  std::memcpy(P->pos, t, sizeof(t));
}
bool ct_align_opts_ok(const wc_map_ct_align_opts *o) {
  return o && o->max_iterations >= 1 && o->tol_rot > 0.0 && o->tol_trans > 0.0 && o->min_used >= 12 && o->min_pivot > 0.0 && ct_prior_ok(o->prior);
}
double norm3(const double *x) { return std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); }
}  // namespace

extern "C" int wc_map_linearize_ct(wc_ctx *ctx, wc_map *m, const wc_points *pts, const wc_pose *pose_begin, const wc_pose *pose_end,
                                   double t_begin, double t_end, const wc_map_reg_params *params, wc_map_ct_normal_eq *h_out,
                                   wc_map_ct_row *d_rows, float *d_xyz_out) {
  wc_dev_guard dg_(ctx);
  map_ct_pose C;
  if (!ct_args_ok(ctx, m, pts, params) || !h_out || (uintptr_t)d_rows % 8 || (uintptr_t)d_xyz_out % 4 ||
      !ct_pose_of(pose_begin, pose_end, t_begin, t_end, &C))
    return wc_fail(ctx, WC_ERR_ARG, kCtArgsMsg, __func__);
  return ct_lin_core(ctx, m, pts, C, params, h_out, d_rows, d_xyz_out, __func__);
}

extern "C" int wc_map_align_ct(wc_ctx *ctx, wc_map *m, const wc_points *pts, wc_pose *pose_begin_io, wc_pose *pose_end_io, double t_begin,
                               double t_end, const wc_map_ct_align_opts *o, wc_map_ct_align_summary *s) {
  wc_dev_guard dg_(ctx);
  if (!ctx || !s || !ct_align_opts_ok(o))
    return wc_fail(ctx, WC_ERR_ARG,
                   "%s: null or out-of-range argument (max_iterations >= 1, tol_rot, tol_trans, min_pivot > 0, min_used >= 12, prior >= 0)", __func__);
  map_ct_pose C;
  if (!ct_args_ok(ctx, m, pts, &o->reg) || !ct_pose_of(pose_begin_io, pose_end_io, t_begin, t_end, &C))
    return wc_fail(ctx, WC_ERR_ARG, kCtArgsMsg, __func__);
  std::memset(s, 0, sizeof(*s));
  s->termination = 1;
  double acc[12] = {};
  wc_map_ct_normal_eq ne;
  bool fresh = false;  // ne is the linearisation at the poses as they stand
  for (uint32_t it = 0; it < o->max_iterations; ++it) {
    if (!ct_pose_of(pose_begin_io, pose_end_io, t_begin, t_end, &C)) return wc_fail(ctx, WC_ERR_NUMERIC, "%s: an update left an unusable pose", __func__);
    WC_TRY(ct_lin_core(ctx, m, pts, C, &o->reg, &ne, nullptr, nullptr, __func__));
    fresh = true;
    if (it == 0) s->initial_cost = ne.cost;
    double xi[12];
    if (ne.n_used < o->min_used || !ct_step(ne, o->prior, acc, o->min_pivot, xi)) {
      s->termination = 2;
      break;
    }
    wc_pose b = *pose_begin_io, e = *pose_end_io;
    ct_pose_update(&b, xi), ct_pose_update(&e, xi + 6);
    map_ct_pose C2;
    if (!ct_pose_of(&b, &e, t_begin, t_end, &C2)) {  // (a non-finite update)
      s->termination = 2;
      break;
    }
    *pose_begin_io = b, *pose_end_io = e;
    fresh = false;
    for (int j = 0; j < 12; ++j) acc[j] += xi[j];
    std::memcpy(s->last_step, xi, sizeof(xi));
    s->iterations = (int32_t)(it + 1);
    if (norm3(xi) <= o->tol_rot && norm3(xi + 3) <= o->tol_trans && norm3(xi + 6) <= o->tol_rot && norm3(xi + 9) <= o->tol_trans) {
      s->termination = 0;
      break;
    }
  }
  if (!fresh) {
    if (!ct_pose_of(pose_begin_io, pose_end_io, t_begin, t_end, &C)) return wc_fail(ctx, WC_ERR_NUMERIC, "%s: an update left an unusable pose", __func__);
    WC_TRY(ct_lin_core(ctx, m, pts, C, &o->reg, &ne, nullptr, nullptr, __func__));
  }
  s->final_cost = ne.cost;
  s->n_used = ne.n_used, s->n_found = ne.n_found, s->n_outside = ne.n_outside;
  double pc = 0.0;
  for (int j = 0; j < 12; ++j) pc += (o->prior[j / 3] * acc[j]) * acc[j];
  s->prior_cost = 0.5 * pc;
  return WC_OK;
}

extern "C" int wc_pose_interp_move(const wc_pose *pose_begin, const wc_pose *pose_end, double t_begin, double t_end, const float *xyz,
                                   const double *times, uint64_t n, float *xyz_out) {
  map_ct_pose C;
  if ((n && (!xyz || !times || !xyz_out)) || !ct_pose_of(pose_begin, pose_end, t_begin, t_end, &C)) return WC_ERR_ARG;
  for (uint64_t i = 0; i < n; ++i) {
    double s;
    if (map_ct_share(C, times[i], s)) {
      map_move_ct(C, s, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xyz_out[3 * i], xyz_out[3 * i + 1], xyz_out[3 * i + 2]);
    } else {
      for (int a = 0; a < 3; ++a) std::memcpy(&xyz_out[3 * i + a], &kCtNaN, 4);
    }
  }
  return WC_OK;
}

extern "C" int wc_map_ct_step(const wc_map_ct_normal_eq *ne, const double prior[4], const double acc[12], double min_pivot, double xi12[12]) {
  if (!ne || !prior || !acc || !xi12 || !(min_pivot > 0.0) || !ct_prior_ok(prior)) return WC_ERR_ARG;
  double xi[12];
  if (!ct_step(*ne, prior, acc, min_pivot, xi)) return WC_ERR_NUMERIC;
  std::memcpy(xi12, xi, sizeof(xi));
  return WC_OK;
}

// ---- the winner of a batch and yaw hypotheses: host only, no context (include/wildcat_hip.h) ------------------------------------------
extern "C" int wc_map_align_best(const wc_map_align_summary *s, const int32_t *status, uint32_t K, uint64_t min_used, int32_t *best) {
  if (!best || (K && (!s || !status))) return WC_ERR_ARG;
  *best = -1;
  for (uint32_t h = 0; h < K; ++h) {
    if (status[h] != WC_OK || s[h].termination == 2 || s[h].n_used < min_used || !std::isfinite(s[h].final_cost)) continue;
    if (*best < 0 || s[h].n_used > s[*best].n_used || (s[h].n_used == s[*best].n_used && s[h].final_cost < s[*best].final_cost)) *best = (int32_t)h;
  }
  return WC_OK;
}

extern "C" int wc_pose_yaw_grid(const double T0[12], uint32_t K, double *T_out) {
  if (!T0 || (K && !T_out)) return WC_ERR_ARG;
  for (uint32_t k = 0; k < K; ++k) {
    double *T = T_out + 12 * (size_t)k;
    std::memcpy(T, T0, 12 * sizeof(double));
    if (k == 0) continue;
    // the angle, its sine and cosine in long double, each rounded to double once: exact to half an ulp of a double
    const long double ang = (2.0L * 3.14159265358979323846264338327950288L * (long double)k) / (long double)K;
    const double c = (double)cosl(ang), sn = (double)sinl(ang);
    for (int j = 0; j < 3; ++j) {
      T[j] = c * T0[j] - sn * T0[4 + j];
      T[4 + j] = sn * T0[j] + c * T0[4 + j];
    }
  }
  return WC_OK;
}

// ---- occupancy score of pose hypotheses (include/wildcat_hip.h: wc_map_score_batch, wc_pose_grid, wc_map_score_top) ------
namespace {
constexpr uint32_t kScoreMaxK = 1u << 20;        // hypotheses of one call, and poses of one wc_pose_grid
constexpr uint64_t kScoreMaxPairs = 1ull << 34;  // (point, pose) pairs of one call: both are design caps
}  // namespace

extern "C" int wc_map_score_batch(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double *T, uint32_t K, const wc_map_score_params *params,
                                  wc_map_score *h_out) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !map_points_ok(pts) || !params || params->min_points == 0 || params->reserved != 0 || (K && (!T || !h_out)) ||
      pts->n >= ((uint64_t)1 << 31) || K > kScoreMaxK)
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument (n < 2^31, K <= 2^20, min_points >= 1, reserved = 0), or a map of another context",
                   __func__);
  WC_TRY(poses_finite(ctx, T, K, __func__));
  if ((uint64_t)K * pts->n > kScoreMaxPairs) return wc_fail(ctx, WC_ERR_CAPACITY, "%s: K * n exceeds 2^34", __func__);
  if (K == 0) return WC_OK;
  if (pts->n == 0) {
    std::memset(h_out, 0, (size_t)K * sizeof(*h_out));
    return WC_OK;
  }
  const size_t cnt_bytes = (size_t)K * sizeof(wc_map_score), pose_bytes = (size_t)K * 12 * sizeof(double);
  WC_TRY(wc_ensure(ctx, m->b_score, cnt_bytes + pose_bytes));
  if (m->h_score_cap < K) {
    if (m->h_score) (void)hipHostFree(m->h_score);
    m->h_score = nullptr, m->h_score_cap = 0;
    WC_HIP(ctx, hipHostMalloc((void **)&m->h_score, cnt_bytes + pose_bytes));
    m->h_score_cap = K;
  }
  unsigned *d_cnt = (unsigned *)m->b_score.p;
  double *d_pose = (double *)((unsigned char *)m->b_score.p + cnt_bytes);
  std::memcpy(m->h_score + cnt_bytes, T, pose_bytes);
  WC_HIP(ctx, hipMemcpyAsync(d_pose, m->h_score + cnt_bytes, pose_bytes, hipMemcpyHostToDevice, ctx->stream));
  WC_HIP(ctx, hipMemsetAsync(d_cnt, 0, cnt_bytes, ctx->stream));
  const uint64_t tiles = (pts->n + kScoreThreads - 1) / kScoreThreads, items = (uint64_t)((K + kScoreBlock - 1) / kScoreBlock) * tiles;
  uint64_t grid = std::min<uint64_t>(items, (uint64_t)8 * m->cus);
  if (ctx->dev.map_score_groups > 0) grid = std::min<uint64_t>(items, (uint64_t)ctx->dev.map_score_groups);  // (development option)
  k_map_score_batch<kScoreBatch><<<(unsigned)grid, kScoreThreads, 0, ctx->stream>>>(*pts, d_pose, K, m->voxel, m->keys, m->pay, m->cap - 1,
                                                                                   params->min_points, d_cnt);
  WC_HIP(ctx, hipGetLastError());
  WC_HIP(ctx, hipMemcpyAsync(m->h_score, d_cnt, cnt_bytes, hipMemcpyDeviceToHost, ctx->stream));
  WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(h_out, m->h_score, cnt_bytes);
  return WC_OK;
}

extern "C" int wc_pose_grid(const double T0[12], uint32_t n_yaw, const uint32_t n[3], const double step[3], double *T_out) {
  if (!T0 || !n || !step || !T_out) return WC_ERR_ARG;
  uint64_t K = n_yaw;
  for (int a = 0; a < 3; ++a) {
    if (K == 0 || K > kScoreMaxK || n[a] == 0 || !(step[a] >= 0.0) || !std::isfinite(step[a])) return WC_ERR_ARG;
    K *= n[a];  // (at most 2^20 * 2^32)
  }
  if (K > kScoreMaxK) return WC_ERR_ARG;
  for (int j = 0; j < 12; ++j)
    if (!std::isfinite(T0[j])) return WC_ERR_ARG;
  std::vector<double> rot((size_t)n_yaw * 12);
  if (wc_pose_yaw_grid(T0, n_yaw, rot.data()) != WC_OK) return WC_ERR_ARG;
  double *T = T_out;
  for (uint32_t k = 0; k < n_yaw; ++k)
    for (uint32_t i0 = 0; i0 < n[0]; ++i0)
      for (uint32_t i1 = 0; i1 < n[1]; ++i1)
        for (uint32_t i2 = 0; i2 < n[2]; ++i2, T += 12) {
          const uint32_t i[3] = {i0, i1, i2};
          std::memcpy(T, rot.data() + (size_t)k * 12, 12 * sizeof(double));
          for (int a = 0; a < 3; ++a)  // (2 i - (n - 1) is an exact integer, its half exact: one rounded product, one rounded sum)
            T[4 * a + 3] = T0[4 * a + 3] + ((double)(2 * (int64_t)i[a] - ((int64_t)n[a] - 1)) * 0.5) * step[a];
        }
  return WC_OK;
}

extern "C" int wc_map_score_top(const wc_map_score *scores, uint32_t K, uint32_t M, uint32_t min_hit, int32_t *idx_out, uint32_t *n_out) {
  if (!n_out || (K && !scores) || (M && !idx_out)) return WC_ERR_ARG;
  std::vector<uint32_t> ok;
  for (uint32_t h = 0; h < K; ++h)
    if (scores[h].n_bad == 0 && scores[h].n_hit >= min_hit) ok.push_back(h);
  const size_t take = std::min<size_t>(M, ok.size());
  std::partial_sort(ok.begin(), ok.begin() + take, ok.end(),
                    [&](uint32_t a, uint32_t b) { return scores[a].n_hit != scores[b].n_hit ? scores[a].n_hit > scores[b].n_hit : a < b; });
  for (uint32_t j = 0; j < M; ++j) idx_out[j] = j < take ? (int32_t)ok[j] : -1;
  *n_out = (uint32_t)take;
  return WC_OK;
}

extern "C" int wc_map_crop(wc_ctx *ctx, wc_map *m, const double lo[3], const double hi[3], uint64_t *h_removed_voxels) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !lo || !hi) return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument", __func__);
  map_sel_box box;
  for (int a = 0; a < 3; ++a) {
    if (!(lo[a] <= hi[a])) return wc_fail(ctx, WC_ERR_ARG, "%s: NaN bound or lo > hi on axis %d", __func__, a);
    // kept: floor(lo / v) <= k <= floor(hi / v), clamped to the key range |k| < 2^20 (+-inf included)
    box.lo[a] = (int)std::min(std::max(std::floor(lo[a] / m->voxel), -(kMapKeyLim - 1.0)), kMapKeyLim);
    box.hi[a] = (int)std::min(std::max(std::floor(hi[a] / m->voxel), -kMapKeyLim), kMapKeyLim - 1.0);
  }
  WC_HIP(ctx, hipMemsetAsync(m->ctr + kCtrKeepVox, 0, (kCtrKeepPts - kCtrKeepVox + 1) * 8, ctx->stream));
  const unsigned grid = (unsigned)std::min<uint64_t>((m->cap + 255) / 256, (uint64_t)8 * m->cus);
  k_map_count<<<grid, 256, 0, ctx->stream>>>(m->keys, m->pay, m->cap, box, m->ctr + kCtrKeepVox, m->ctr + kCtrKeepPts);
  WC_HIP(ctx, hipGetLastError());
  WC_TRY(map_sync_counters(ctx, m));  // (the wait: the new table is sized from the kept count; a pending counter copy has landed too)
  const uint64_t occ = m->h_ctr[kCtrOcc], kept = m->h_ctr[kCtrKeepVox], kept_pts = m->h_ctr[kCtrKeepPts];
  if (h_removed_voxels) *h_removed_voxels = occ - kept;
  const uint64_t cap = pow2_at_least(2 * std::max<uint64_t>(kept, 1));
  if (kept != occ || cap != m->cap) {  // (otherwise the table already is what the crop would build)
    WC_TRY(map_replace_table(ctx, m, cap, box));
    m->tombs = 0;  // (a replacement: the rehash leaves the tombstones behind)
    // the occupied-voxel and point counters become those of the kept voxels; rejected and growth counters stay
    WC_HIP(ctx, hipMemcpyAsync(m->ctr + kCtrOcc, m->ctr + kCtrKeepVox, 8, hipMemcpyDeviceToDevice, ctx->stream));
    WC_HIP(ctx, hipMemcpyAsync(m->ctr + kCtrPts, m->ctr + kCtrKeepPts, 8, hipMemcpyDeviceToDevice, ctx->stream));
    m->h_ctr[kCtrOcc] = kept, m->h_ctr[kCtrPts] = kept_pts;
  }
  // the growth policy starts again from the exact count (map_sync_counters has cleared the pending copy)
  m->occ_known = kept;
  m->pts_since = m->pts_after_copy = 0;
  return WC_OK;
}

// ---- carving free space along a sweep's rays (include/wildcat_hip.h: wc_map_carve) -------------------------------------------------
namespace {
// wc_map_carve (remove = false: the map is left as it is) and wc_map_carve_remove: one definition, one ray kernel; the slot pass counts
// (k_map_count) or counts and erases (k_map_erase)
int map_carve(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double origin[3], const wc_map_carve_params *params, wc_map_carve_result *h_out,
              bool remove, const char *fn) {
  wc_dev_guard dg_(ctx);
  const wc_map_carve_params *p = params;
  if (!map_ok(ctx, m) || !map_points_ok(pts) || !origin || !p || !h_out || pts->n >= ((uint64_t)1 << 31))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument (n < 2^31), or a map of another context", fn);
  if (!(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])) || !(p->min_range >= 0.0) ||
      !(p->max_range >= p->min_range) || p->shell > 8 || p->min_rays < 1 || p->max_steps < 1 || p->max_steps > 65536 || p->reserved != 0)
    return wc_fail(ctx, WC_ERR_ARG,
                   "%s: origin not finite, or params out of range (0 <= min_range <= max_range, shell <= 8, min_rays >= 1, 1 <= max_steps <= 65536, "
                   "reserved = 0)",
                   fn);
  std::memset(h_out, 0, sizeof(*h_out));
  if (pts->n == 0) return WC_OK;  // (no ray, no end mark: nothing is removed and nothing is launched)
  map_ray_args A;
  A.v = m->voxel;
  A.min2 = p->min_range * p->min_range, A.max2 = p->max_range * p->max_range;
  for (int a = 0; a < 3; ++a) A.o[a] = origin[a];
  A.k0_ok = map_voxel_of(origin[0], origin[1], origin[2], m->voxel, A.k0[0], A.k0[1], A.k0[2]) ? 1u : 0u;
  A.shell = p->shell, A.max_steps = p->max_steps;
  // the scratch: five counter lines, then one word per slot; zeroed per call
  const size_t scratch = (size_t)kCarveCtrWords * 8 + (size_t)m->cap * 4;
  WC_TRY(wc_ensure(ctx, m->b_carve, scratch));
  if (!m->h_carve) WC_HIP(ctx, hipHostMalloc((void **)&m->h_carve, kCarveCtrWords * 8));
  unsigned long long *cctr = (unsigned long long *)m->b_carve.p;
  unsigned *words = (unsigned *)(cctr + kCarveCtrWords);
  WC_HIP(ctx, hipMemsetAsync(m->b_carve.p, 0, scratch, ctx->stream));
  const uint64_t blocks = (pts->n + kCarveThreads - 1) / kCarveThreads;
  uint64_t grid = std::min<uint64_t>(blocks, (uint64_t)8 * m->cus);
  if (ctx->dev.map_carve_groups > 0) grid = std::min<uint64_t>(blocks, (uint64_t)ctx->dev.map_carve_groups);  // (development option)
  k_map_carve<kCarveBatch><<<(unsigned)grid, kCarveThreads, 0, ctx->stream>>>(*pts, A, m->keys, m->cap - 1, words, cctr);
  WC_HIP(ctx, hipGetLastError());
  // what the words select: counted, or counted and erased in the same pass
  const unsigned cgrid = (unsigned)std::min<uint64_t>((m->cap + 255) / 256, (uint64_t)8 * m->cus);
  if (remove)
    k_map_erase<<<cgrid, 256, 0, ctx->stream>>>(m->keys, m->pay, m->cap, map_sel_carve{words, p->min_rays}, cctr + kCarveSelVox,
                                                cctr + kCarveSelPts, m->ctr);
  else
    k_map_count<<<cgrid, 256, 0, ctx->stream>>>(m->keys, m->pay, m->cap, map_sel_carve{words, p->min_rays}, cctr + kCarveSelVox,
                                                cctr + kCarveSelPts);
  WC_HIP(ctx, hipGetLastError());
  WC_HIP(ctx, hipMemcpyAsync(m->h_carve, cctr, kCarveCtrWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (remove)
    WC_TRY(map_sync_counters(ctx, m));  // (the wait; the map's counters are exact again and a pending copy has landed)
  else
    WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  h_out->rays_used = m->h_carve[kCarveUsed], h_out->rays_skipped = m->h_carve[kCarveSkip], h_out->steps = m->h_carve[kCarveSteps];
  h_out->voxels_removed = m->h_carve[kCarveSelVox], h_out->points_removed = m->h_carve[kCarveSelPts];
  if (remove) m->tombs += m->h_carve[kCarveSelVox];
  return WC_OK;
}
}  // namespace

extern "C" int wc_map_carve(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double origin[3], const wc_map_carve_params *params,
                            wc_map_carve_result *h_out) {
  return map_carve(ctx, m, pts, origin, params, h_out, false, __func__);
}

// ---- removal in place (include/wildcat_hip.h: wc_map_carve_remove, wc_map_remove_keys, wc_map_tombstones) ---------------
extern "C" int wc_map_carve_remove(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double origin[3], const wc_map_carve_params *params,
                                   wc_map_carve_result *h_out) {
  return map_carve(ctx, m, pts, origin, params, h_out, true, __func__);
}

extern "C" int wc_map_remove_keys(wc_ctx *ctx, wc_map *m, const int32_t *d_keys, uint64_t n, uint64_t h_out[3]) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !h_out) return wc_fail(ctx, WC_ERR_ARG, "%s: null argument or a map of another context", __func__);
  h_out[0] = h_out[1] = h_out[2] = 0;
  if (n == 0) return WC_OK;
  if (!d_keys || (uintptr_t)d_keys % 4 || n > ((uint64_t)1 << 31))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or misaligned keys, or n > 2^31", __func__);
  WC_HIP(ctx, hipMemsetAsync(m->ctr + kCtrRmVox, 0, (kCtrRmNone - kCtrRmVox + 1) * 8, ctx->stream));
  const uint64_t blocks = (n + kRemoveThreads - 1) / kRemoveThreads;
  uint64_t grid = std::min<uint64_t>(blocks, (uint64_t)8 * m->cus);
  if (ctx->dev.map_remove_groups > 0) grid = std::min<uint64_t>(blocks, (uint64_t)ctx->dev.map_remove_groups);  // (development option)
  k_map_remove_keys<<<(unsigned)grid, kRemoveThreads, 0, ctx->stream>>>(d_keys, n, m->keys, m->pay, m->cap - 1, m->ctr);
  WC_HIP(ctx, hipGetLastError());
  WC_TRY(map_sync_counters(ctx, m));  // (the wait: the call's three counters travel with the map's)
  h_out[0] = m->h_ctr[kCtrRmVox], h_out[1] = m->h_ctr[kCtrRmPts], h_out[2] = m->h_ctr[kCtrRmNone];
  m->tombs += h_out[0];
  return WC_OK;
}

extern "C" int wc_map_tombstones(wc_ctx *ctx, wc_map *m, uint64_t h_out[2]) {
  if (!map_ok(ctx, m) || !h_out) return wc_fail(ctx, WC_ERR_ARG, "%s: null argument or a map of another context", __func__);
  h_out[0] = m->tombs, h_out[1] = m->purges;
  return WC_OK;
}

// ---- casting rays to their first occupied voxel (include/wildcat_hip.h: wc_map_raycast) --------------------------------------------
extern "C" int wc_map_raycast(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double origin[3], const wc_map_raycast_params *params,
                              wc_map_ray_hit *d_hits, wc_map_raycast_result *h_out) {
  wc_dev_guard dg_(ctx);
  const wc_map_raycast_params *p = params;
  if (!map_ok(ctx, m) || !map_points_ok(pts) || !origin || !p || pts->n >= ((uint64_t)1 << 31) || (pts->n && (!d_hits || (uintptr_t)d_hits % 8)))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or out-of-range argument (n < 2^31, d_hits 8-aligned), or a map of another context", __func__);
  if (!(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])) || !(p->min_range >= 0.0) ||
      !(p->max_range >= p->min_range) || p->first_step > 65536 || p->end_shell > 9 || p->min_points < 1 || p->max_steps < 1 || p->max_steps > 65536)
    return wc_fail(ctx, WC_ERR_ARG,
                   "%s: origin not finite, or params out of range (0 <= min_range <= max_range, first_step <= 65536, end_shell <= 9, "
                   "min_points >= 1, 1 <= max_steps <= 65536)",
                   __func__);
  if (h_out) std::memset(h_out, 0, sizeof(*h_out));
  if (pts->n == 0) return WC_OK;  // (no ray: nothing is launched)
  map_ray_args A;
  A.v = m->voxel;
  A.min2 = p->min_range * p->min_range, A.max2 = p->max_range * p->max_range;
  for (int a = 0; a < 3; ++a) A.o[a] = origin[a];
  A.k0_ok = map_voxel_of(origin[0], origin[1], origin[2], m->voxel, A.k0[0], A.k0[1], A.k0[2]) ? 1u : 0u;
  A.shell = p->end_shell, A.max_steps = p->max_steps;
  // the call's own four counter lines, zeroed per call: neither the map nor any scratch of another call is written
  WC_TRY(wc_ensure(ctx, m->b_cast, (size_t)kCastCtrWords * 8));
  if (!m->h_cast) WC_HIP(ctx, hipHostMalloc((void **)&m->h_cast, kCastCtrWords * 8));
  unsigned long long *cctr = (unsigned long long *)m->b_cast.p;
  WC_HIP(ctx, hipMemsetAsync(cctr, 0, (size_t)kCastCtrWords * 8, ctx->stream));
  const uint64_t blocks = (pts->n + kCastThreads - 1) / kCastThreads;
  uint64_t grid = std::min<uint64_t>(blocks, (uint64_t)8 * m->cus);
  if (ctx->dev.map_cast_groups > 0) grid = std::min<uint64_t>(blocks, (uint64_t)ctx->dev.map_cast_groups);  // (development option)
  k_map_raycast<kCastBatch><<<(unsigned)grid, kCastThreads, 0, ctx->stream>>>(*pts, A, p->first_step, p->min_points, m->keys, m->pay, m->cap - 1,
                                                                             d_hits, cctr);
  WC_HIP(ctx, hipGetLastError());
  if (h_out) {
    WC_HIP(ctx, hipMemcpyAsync(m->h_cast, cctr, kCastCtrWords * 8, hipMemcpyDeviceToHost, ctx->stream));
    WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h_out->rays_cast = m->h_cast[kCastCast], h_out->rays_skipped = m->h_cast[kCastSkip];
    h_out->hits = m->h_cast[kCastHits], h_out->tested = m->h_cast[kCastTested];
  }
  return WC_OK;
}

// ---- connected components (include/wildcat_hip.h: wc_map_components, wc_map_remove_small, wc_map_label_keys) -------------
namespace {
bool cc_params_ok(const wc_map_cc_params *p) {
  return p && (p->connectivity == 6 || p->connectivity == 18 || p->connectivity == 26) && p->min_points >= 1 &&
         !(p->flags & ~(uint32_t)WC_MAP_CC_DROP_SPARSE) && p->reserved == 0;
}
constexpr const char *kCcParamsText = "connectivity 6, 18 or 26, min_points >= 1, flags: WC_MAP_CC_DROP_SPARSE, reserved = 0";

// what one run of the labelling leaves in the map's scratch, until the next call that uses it
struct cc_run {
  uint64_t n = 0, nodes = 0, comps = 0, largest = 0;
  unsigned long long *skeys = nullptr;  // the export's sorted pairs
  uint32_t *sslots = nullptr;
  unsigned long long *cctr = nullptr;
  uint32_t *root = nullptr, *num = nullptr, *sel = nullptr;
  wc_map_component *d_comps = nullptr;
  unsigned grid = 1;
};
unsigned cc_grid(const wc_ctx *ctx, const wc_map *m, uint64_t items) {
  const uint64_t blocks = std::max<uint64_t>((items + kCcThreads - 1) / kCcThreads, 1);
  uint64_t grid = std::min<uint64_t>(blocks, (uint64_t)8 * m->cus);
  if (ctx->dev.map_cc_groups > 0) grid = std::min<uint64_t>(blocks, (uint64_t)ctx->dev.map_cc_groups);  // (development option)
  return (unsigned)grid;
}
// the labelling of the map as it stands: index, link, flatten, scan, then - the component count read back - records and the largest.
// d_label / d_keys (either may be NULL) are written by the stats pass; want_sel: the selection words of wc_map_remove_small.  Waits twice
int cc_core(wc_ctx *ctx, wc_map *m, const wc_map_cc_params *p, uint32_t *d_label, int32_t *d_keys, bool want_sel, uint32_t min_voxels,
            uint64_t min_comp_points, cc_run *R, const char *fn) {
  WC_TRY(map_sync_counters(ctx, m));
  const uint64_t n = R->n = m->h_ctr[kCtrOcc];
  if (n == 0) return WC_OK;
  WC_TRY(map_sorted_slots(ctx, m, n, &R->skeys, &R->sslots));
  WC_TRY(wc_ensure(ctx, m->b_cc_idx, (size_t)m->cap * 4));
  WC_TRY(wc_ensure(ctx, m->b_cc, (size_t)kCcCtrWords * 8 + (size_t)n * 16));
  if (!m->h_cc) WC_HIP(ctx, hipHostMalloc((void **)&m->h_cc, kCcCtrWords * 8));
  unsigned long long *cctr = R->cctr = (unsigned long long *)m->b_cc.p;
  uint32_t *idx = (uint32_t *)m->b_cc_idx.p, *parent = (uint32_t *)(cctr + kCcCtrWords), *root = parent + n, *flag = root + n, *num = flag + n;
  R->root = root, R->num = num;
  WC_HIP(ctx, hipMemsetAsync(cctr, 0, (size_t)kCcCtrWords * 8, ctx->stream));
  const unsigned grid = R->grid = cc_grid(ctx, m, n);
  k_map_cc_index<<<grid, kCcThreads, 0, ctx->stream>>>(R->sslots, n, m->pay, p->min_points, idx, parent, cctr);
  WC_HIP(ctx, hipGetLastError());
  const unsigned long long budget = 8ull * n + 64;
  if (p->connectivity == 6)
    k_map_cc_link<3><<<grid, kCcThreads, 0, ctx->stream>>>(R->skeys, n, m->keys, m->cap - 1, idx, parent, budget, cctr + kCcErr);
  else if (p->connectivity == 18)
    k_map_cc_link<9><<<grid, kCcThreads, 0, ctx->stream>>>(R->skeys, n, m->keys, m->cap - 1, idx, parent, budget, cctr + kCcErr);
  else
    k_map_cc_link<13><<<grid, kCcThreads, 0, ctx->stream>>>(R->skeys, n, m->keys, m->cap - 1, idx, parent, budget, cctr + kCcErr);
  WC_HIP(ctx, hipGetLastError());
  k_map_cc_flatten<<<grid, kCcThreads, 0, ctx->stream>>>(parent, n, root, flag, cctr);
  WC_HIP(ctx, hipGetLastError());
  size_t tmp = 0;
  WC_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp, flag, num, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->stream));
  WC_TRY(wc_ensure(ctx, m->b_cc_tmp, tmp));
  tmp = m->b_cc_tmp.cap;
  WC_HIP(ctx, rocprim::exclusive_scan(m->b_cc_tmp.p, tmp, flag, num, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->stream));
  WC_HIP(ctx, hipMemcpyAsync(m->h_cc, cctr, kCcCtrWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  WC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the first wait: the records' buffer is sized from the component count)
  if (m->h_cc[kCcErr])
    return wc_fail(ctx, WC_ERR_INTERNAL, "%s: %llu lanes of the labelling ran past their loop bound (the map is untouched)", fn, m->h_cc[kCcErr]);
  R->nodes = m->h_cc[kCcNodes];
  const uint64_t C = R->comps = m->h_cc[kCcComps];
  WC_TRY(wc_ensure(ctx, m->b_cc_comps, (size_t)std::max<uint64_t>(C, 1) * (sizeof(wc_map_component) + 4)));
  R->d_comps = (wc_map_component *)m->b_cc_comps.p;
  R->sel = (uint32_t *)(R->d_comps + std::max<uint64_t>(C, 1));
  if (C) {
    k_map_cc_clear<<<cc_grid(ctx, m, C), kCcThreads, 0, ctx->stream>>>(R->d_comps, C);
    WC_HIP(ctx, hipGetLastError());
  }
  if (C || d_label || d_keys) {
    // (two wavefronts per CU, each on a contiguous run of tiles: the fewer wavefronts, the fewer atomics on a large component's record)
    unsigned sgrid = (unsigned)std::min<uint64_t>(grid, (uint64_t)std::max(m->cus / 2, 1));
    if (ctx->dev.map_cc_groups > 0) sgrid = grid;
    k_map_cc_stats<<<sgrid, kCcThreads, 0, ctx->stream>>>(R->skeys, R->sslots, n, m->pay, root, num, d_label, d_keys, R->d_comps);
    WC_HIP(ctx, hipGetLastError());
  }
  if (C) {
    k_map_cc_select<<<cc_grid(ctx, m, C), kCcThreads, 0, ctx->stream>>>(R->d_comps, C, min_voxels, min_comp_points, want_sel ? R->sel : nullptr, cctr);
    WC_HIP(ctx, hipGetLastError());
    WC_HIP(ctx, hipMemcpyAsync(m->h_cc, cctr, kCcCtrWords * 8, hipMemcpyDeviceToHost, ctx->stream));
    WC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    R->largest = m->h_cc[kCcLargest];
  }
  return WC_OK;
}
}  // namespace

extern "C" int wc_map_components(wc_ctx *ctx, wc_map *m, const wc_map_cc_params *params, int32_t *d_keys, uint32_t *d_label, uint64_t cap,
                                 wc_map_component *d_comps, uint64_t cap_comps, uint64_t h_out[4]) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !h_out || (uintptr_t)d_keys % 4 || (uintptr_t)d_label % 4 || (uintptr_t)d_comps % 8 || (cap && !d_label))
    return wc_fail(ctx, WC_ERR_ARG, "%s: null or misaligned argument, cap > 0 without d_label, or a map of another context", __func__);
  if (!cc_params_ok(params)) return wc_fail(ctx, WC_ERR_ARG, "%s: params out of range (%s)", __func__, kCcParamsText);
  h_out[0] = h_out[1] = h_out[2] = h_out[3] = 0;
  WC_TRY(map_sync_counters(ctx, m));
  const uint64_t n = m->h_ctr[kCtrOcc];
  if (n == 0) return WC_OK;
  const bool fits = cap >= n;
  cc_run R;
  WC_TRY(cc_core(ctx, m, params, fits ? d_label : nullptr, fits ? d_keys : nullptr, false, 0, 0, &R, __func__));
  h_out[0] = R.n, h_out[1] = R.nodes, h_out[2] = R.comps, h_out[3] = R.largest;
  const bool comps_fit = !d_comps || cap_comps >= R.comps;
  if (d_comps && comps_fit && R.comps)
    WC_HIP(ctx, hipMemcpyAsync(d_comps, R.d_comps, (size_t)R.comps * sizeof(wc_map_component), hipMemcpyDeviceToDevice, ctx->stream));
  WC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the call waits: labels, keys and records are there on return)
  if (!fits) return wc_fail(ctx, WC_ERR_CAPACITY, "%s: %llu voxels, capacity %llu", __func__, (unsigned long long)n, (unsigned long long)cap);
  if (!comps_fit)
    return wc_fail(ctx, WC_ERR_CAPACITY, "%s: %llu components, capacity %llu", __func__, (unsigned long long)R.comps, (unsigned long long)cap_comps);
  return WC_OK;
}

extern "C" int wc_map_remove_small(wc_ctx *ctx, wc_map *m, const wc_map_cc_params *params, uint32_t min_voxels, uint64_t min_comp_points,
                                   uint64_t h_out[4]) {
  wc_dev_guard dg_(ctx);
  if (!map_ok(ctx, m) || !h_out) return wc_fail(ctx, WC_ERR_ARG, "%s: null argument or a map of another context", __func__);
  if (!cc_params_ok(params)) return wc_fail(ctx, WC_ERR_ARG, "%s: params out of range (%s)", __func__, kCcParamsText);
  h_out[0] = h_out[1] = h_out[2] = h_out[3] = 0;
  cc_run R;
  WC_TRY(cc_core(ctx, m, params, nullptr, nullptr, true, min_voxels, min_comp_points, &R, __func__));
  h_out[0] = R.comps;
  const unsigned drop = (params->flags & WC_MAP_CC_DROP_SPARSE) ? 1u : 0u;
  const uint64_t sel_comps = R.comps ? m->h_cc[kCcRmComps] : 0;
  if (R.n == 0 || (!sel_comps && !(drop && R.nodes < R.n))) return WC_OK;  // (nothing selected: nothing is launched, no tombstone is written)
  k_map_cc_erase<<<R.grid, kCcThreads, 0, ctx->stream>>>(R.sslots, R.n, R.root, R.num, R.sel, drop, m->keys, m->pay, R.cctr, m->ctr);
  WC_HIP(ctx, hipGetLastError());
  WC_HIP(ctx, hipMemcpyAsync(m->h_cc, R.cctr, kCcCtrWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  WC_TRY(map_sync_counters(ctx, m));  // (the wait; the map's counters are exact again and a pending copy has landed)
  h_out[1] = sel_comps, h_out[2] = m->h_cc[kCcRmVox], h_out[3] = m->h_cc[kCcRmPts];
  m->tombs += h_out[2];
  return WC_OK;
}

extern "C" int wc_map_label_keys(const int32_t *keys, const uint32_t *count, uint64_t n, const wc_map_cc_params *params, uint32_t *label_out,
                                 wc_map_component *comps_out, uint64_t cap_comps, uint64_t h_out[4]) {
  if (!h_out || !cc_params_ok(params) || n > ((uint64_t)1 << 31) || (n && (!keys || !count || !label_out))) return WC_ERR_ARG;
  auto pack = [](int kx, int ky, int kz) {
    return ((uint64_t)(kx + kMapKeyOff) << 42) | ((uint64_t)(ky + kMapKeyOff) << 21) | (uint64_t)(kz + kMapKeyOff);
  };
  std::vector<uint64_t> pk(n);
  for (uint64_t i = 0; i < n; ++i) {
    const int32_t *k = keys + 3 * i;
    if (!cc_in_range(k[0]) || !cc_in_range(k[1]) || !cc_in_range(k[2])) return WC_ERR_ARG;
    pk[i] = pack(k[0], k[1], k[2]);
    if (i && pk[i] <= pk[i - 1]) return WC_ERR_ARG;  // (unsorted, or a key twice)
  }
  // union-find over the export order: the larger root under the smaller, so a component's root is its smallest index
  std::vector<uint32_t> parent(n);
  uint64_t nodes = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const bool node = count[i] >= params->min_points;
    parent[i] = node ? (uint32_t)i : kCcNone;
    nodes += node;
  }
  auto find = [&](uint32_t x) {
    uint32_t r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) {
      const uint32_t nx = parent[x];
      parent[x] = r;
      x = nx;
    }
    return r;
  };
  const int nb = cc_lower(params->connectivity);
  for (uint64_t i = 0; i < n; ++i) {
    if (parent[i] == kCcNone) continue;
    const int32_t *k = keys + 3 * i;
    for (int j = 0; j < nb; ++j) {
      const int x = k[0] + cc_off(j, 0), y = k[1] + cc_off(j, 1), z = k[2] + cc_off(j, 2);
      if (!cc_in_range(x) || !cc_in_range(y) || !cc_in_range(z)) continue;
      const uint64_t q = pack(x, y, z);
      const auto it = std::lower_bound(pk.begin(), pk.begin() + i, q);  // (a lower neighbour: a smaller key, an earlier entry)
      if (it == pk.begin() + i || *it != q) continue;
      const uint32_t o = (uint32_t)(it - pk.begin());
      if (parent[o] == kCcNone) continue;
      const uint32_t a = find((uint32_t)i), b = find(o);
      if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
  }
  std::vector<uint32_t> num(n, kCcNone);
  uint64_t C = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (parent[i] == (uint32_t)i) num[i] = (uint32_t)C++;
  std::vector<uint32_t> vox(C, 0);
  const bool comps_fit = !comps_out || cap_comps >= C;
  const bool write = comps_out && comps_fit;
  for (uint64_t c = 0; write && c < C; ++c) {
    wc_map_component r;
    std::memset(&r, 0, sizeof(r));
    r.kmin[0] = r.kmin[1] = r.kmin[2] = INT32_MAX;
    r.kmax[0] = r.kmax[1] = r.kmax[2] = INT32_MIN;
    comps_out[c] = r;
  }
  uint64_t largest = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (parent[i] == kCcNone) {
      label_out[i] = kCcNone;
      continue;
    }
    const uint32_t r = find((uint32_t)i), c = num[r];
    label_out[i] = c;
    largest = std::max<uint64_t>(largest, ++vox[c]);
    if (!write) continue;
    wc_map_component &o = comps_out[c];
    if (r == (uint32_t)i) o.first = r;
    o.voxels += 1;
    o.points += count[i];
    for (int a = 0; a < 3; ++a) o.kmin[a] = std::min(o.kmin[a], keys[3 * i + a]), o.kmax[a] = std::max(o.kmax[a], keys[3 * i + a]);
  }
  h_out[0] = n, h_out[1] = nodes, h_out[2] = C, h_out[3] = largest;
  return comps_fit ? WC_OK : WC_ERR_CAPACITY;
}
