// match_tree.inc — the matcher's index (included by match.hip): a kd-tree WITH BOUNDING BOXES over the 6-D features
// [centre / 1.0, normal / 5deg] of the targets.  It takes the place of FLANN's KDTreeSingleIndex(leaf 15) that the
// reference builds in KnnSurfelMatcher::BuildIndex (src/odometry/knn_surfel_matcher.cc:3-14, 65-73) and searches exactly
// (SearchParams(-1, 0.0), cc:75-89).  Rounds 1-3 searched a 3-D grid on the centres: the normal half of the metric (5 degrees
// = 1 unit) could not prune, a query of a sparse window looked at ~860 candidates in ~200 rows.  The tree prunes in all six
// dimensions: ~170 points in ~20 leaves behind ~25 node visits for the same query (profiles/dev/sim_tree.py).
//
// Shape: a COMPLETE binary tree of depth D in heap order (node (d, i) = (1 << d) + i), every node a box (6 x [lo, hi], fp32);
// leaf i holds the sorted targets [leaf_begin[i], leaf_begin[i + 1]).  The walk steps three levels at a time: the 8 boxes that
// far below a node are contiguous (384 bytes).  Exactness never depends on how the tree was built - the boxes are formed from what
// the leaves really hold - only the speed does.
// Build (all on the device, no host round trip):
//   top T levels  split planes from a SAMPLE of the node's points (<= 1024 - every k-th point of the call's order in the first
//                 stage, the points whose index is a multiple of m in the later ones -, one workgroup per node of the previous
//                 stage, <= 5 levels per stage: widest dimension of the cell, median of the sample), then every point is routed
//                 through the planes to one of 2^T buckets (~512 points) and scattered bucket-wise (counting sort, LDS-aggregated)
//   bottom        one workgroup per bucket: its keys in registers, put into canonical order (ascending index), then Bd levels of
//                 "sort the block along the widest dimension of its cell, cut in the middle" (bitonic network: register pairs,
//                 wavefront shuffles, LDS only for strides 64 ... 256), leaves of 4 - 8 points; leaf boxes, the boxes of the
//                 bucket's subtree, the sorted copies of the features
//   top boxes     the levels above the buckets, bottom-up
// Everything is deterministic for given inputs (ties by target index), so the ranks of a query-sharded search build the same tree.

constexpr int kKdSample = 1024;    // sample size of a top stage
constexpr int kKdStageMax = 5;     // levels per top stage (>= 32 samples per bucket; one stage of 7 levels instead of 4 + 3: no gain)
constexpr int kKdTopNT = 1024, kKdBotNT = 512;  // threads of k_kd_top / k_kd_bottom (one / up to four keys per thread)
constexpr int kKdBdMax = 7;        // levels below a bucket (128 leaves)
constexpr int kKdTMax = 13;        // levels above the buckets (8192 buckets)
constexpr int kKdPad = 32;         // bucket counters one per 128-byte line (atomics on one line serialise)

struct KdTree {
  const float4 *box;           // heap of boxes, 3 x float4 per node: lo0..lo3 | lo4 lo5 hi0 hi1 | hi2..hi5; empty node: lo0 > hi0
  const uint32_t *leaf_begin;  // 2^D + 1
  const double *sfeat;         // the sorted features in fp64 (what the exact distance is summed from)
  const uint32_t *sorig;       // sorted position -> target index
  int D;                       // depth
};

__device__ __forceinline__ uint32_t f2ord(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o >> 31) ? (o & 0x7FFFFFFFu) : ~o); }

// segment i of level l of n elements: [n i >> l, n (i + 1) >> l)
__device__ __forceinline__ uint32_t seg_lo(uint32_t n, int l, uint32_t i) { return (uint32_t)(((uint64_t)n * i) >> l); }
__device__ __forceinline__ uint32_t seg_of(uint32_t n, int l, uint32_t pos) {
  uint32_t i = (uint32_t)((((uint64_t)pos) << l) / (n ? n : 1u));
  i = min(i, (1u << l) - 1u);
  while (i + 1u < (1u << l) && seg_lo(n, l, i + 1u) <= pos) ++i;
  while (i > 0u && seg_lo(n, l, i) > pos) --i;
  return i;
}

// ---- the sorting core of the build --------------------------------------------------------------------------------------------------
// A workgroup of 256 threads holds P = E x 256 keys in REGISTERS (key e of thread t is element e * 256 + t) and sorts every
// aligned block of B keys (B a power of two) with the bitonic network: strides >= 256 pair two registers of one thread, strides
// below 64 are wavefront shuffles, only strides 64 and 128 go through LDS (one barrier each, two buffers).  The first build of
// this round kept the keys in LDS and paid a barrier and three dependent LDS round trips for EVERY one of the ~260 comparator
// steps of a bucket: ~1000 clocks per step, 110 us per bucket (k_kd_bottom) and 105 - 134 us per sample stage (k_kd_top) by
// rocprofv3 - 0.9 ms of build in front of every search.
// (Round 4, tried: the exchanges at strides 1, 2, 4, 8 as DPP moves - quad permutations, and mirrors composed: a quad reversed and then a
// group of eight is lane ^ 4, a group of eight and then a row lane ^ 8 - instead of __shfl_xor's two ds_bpermute per key, picked by a
// wave-uniform switch on the stride: the same trees, and k_kd_top 39 -> 52 us, k_kd_bottom 44 -> 58 us on the room stream's window.
// __shfl_xor stays.)
constexpr unsigned long long kKdPadKey = ~0ull;

template <int E, int kKdNT, int JE>
__device__ __forceinline__ void kd_local_step(unsigned long long (&key)[E], int tid, uint32_t k, uint32_t B) {
  if constexpr (JE < E) {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if ((e & JE) == 0) {
        const uint32_t pos = (uint32_t)e * kKdNT + (uint32_t)tid;
        const bool up = k >= B || (pos & k) == 0u;
        const unsigned long long a = key[e], b = key[e | JE], lo = a < b ? a : b, hi = a < b ? b : a;
        key[e] = up ? lo : hi;
        key[e | JE] = up ? hi : lo;
      }
  }
}

template <int E, int kKdNT>
__device__ __forceinline__ void kd_block_sort(unsigned long long (&key)[E], int tid, uint32_t B, unsigned long long *xbuf /* 2 x E x NT */) {
  int xb = 0;
  for (uint32_t k = 2; k <= B; k <<= 1) {
    for (uint32_t j = k >> 1; j >= 1; j >>= 1) {
      if (j >= (uint32_t)kKdNT) {
        if (j == (uint32_t)kKdNT)
          kd_local_step<E, kKdNT, 1>(key, tid, k, B);
        else if (j == 2u * kKdNT)
          kd_local_step<E, kKdNT, 2>(key, tid, k, B);
        else
          kd_local_step<E, kKdNT, 4>(key, tid, k, B);
        continue;
      }
      unsigned long long pk[E];
      if (j >= 64u) {
        unsigned long long *xw = xbuf + (size_t)xb * E * kKdNT;
#pragma unroll
        for (int e = 0; e < E; ++e) xw[e * kKdNT + tid] = key[e];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e) pk[e] = xw[((uint32_t)(e * kKdNT + tid)) ^ j];
        xb ^= 1;
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) pk[e] = __shfl_xor(key[e], (int)j);
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const uint32_t pos = (uint32_t)e * kKdNT + (uint32_t)tid;
        const bool up = k >= B || (pos & k) == 0u;
        const bool take_min = ((pos & j) == 0u) == up;
        const unsigned long long a = key[e], b = pk[e];
        key[e] = take_min ? (a < b ? a : b) : (a < b ? b : a);
      }
    }
  }
  __syncthreads();  // (the exchange buffers are free again)
}

struct KdLds {
  float (*sf)[6];             // features of the elements, by slot
  unsigned long long *xbuf;   // 2 x P exchange buffers of the sort; also where a level publishes its sorted keys
  float *cell;                // 2 buffers x 2^(levels - 1) x 12: the cells of the current level's blocks
  int *sdim;                  // per block: the dimension it is cut along
  uint32_t *box12;            // 12 words: the bounding box reduction
};

// bounding box of the n elements (slot = position, n at the front) -> L.cell[0 .. 11] (lo, hi)
template <int E, int kKdNT>
__device__ void kd_root_cell(const KdLds &L, uint32_t n, int tid) {
  if (tid < 12) L.box12[tid] = tid < 6 ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  uint32_t lo[6], hi[6];
  for (int d = 0; d < 6; ++d) lo[d] = 0xFFFFFFFFu, hi[d] = 0u;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t s = (uint32_t)e * kKdNT + (uint32_t)tid;
    if (s < n)
      for (int d = 0; d < 6; ++d) {
        const uint32_t o = f2ord(L.sf[s][d]);
        lo[d] = min(lo[d], o), hi[d] = max(hi[d], o);
      }
  }
  for (int d = 0; d < 6; ++d)
    for (int off = 32; off >= 1; off >>= 1) {
      lo[d] = min(lo[d], (uint32_t)__shfl_xor((int)lo[d], off));
      hi[d] = max(hi[d], (uint32_t)__shfl_xor((int)hi[d], off));
    }
  if ((tid & 63) == 0)
    for (int d = 0; d < 6; ++d) atomicMin(&L.box12[d], lo[d]), atomicMax(&L.box12[6 + d], hi[d]);
  __syncthreads();
  if (tid < 12) L.cell[tid] = n ? ord2f(L.box12[tid]) : 0.f;
  __syncthreads();
}

// `levels` levels of "sort every block along the widest dimension of its cell, cut it in the middle".  In: key[e] = slot of
// element e * 256 + tid (the n elements at the front, padding behind), root cell in L.cell[0 .. 11].  Level l works on aligned
// blocks of P >> l keys: block i holds the elements of segment i - [n i >> l, n (i + 1) >> l) of the order so far - at its front;
// after its sort the upper half of the elements moves to the front of the block's upper half.  Out: block i of level `levels`
// (P >> levels keys) = leaf i, also published in L.xbuf[0 .. P).  kPlanes: the cut of block i of level l is stored as the plane
// of heap node (heap0 << l) + i.
template <int E, int kKdNT, bool kPlanes>
__device__ void kd_sort_levels(unsigned long long (&key)[E], const KdLds &L, uint32_t n, int levels, int tid, uint32_t heap0, int *plane_dim,
                               double *plane_val) {
  constexpr uint32_t P = (uint32_t)E * kKdNT;
  const int half = levels > 0 ? (1 << (levels - 1)) : 1;
  int cur = 0;
  for (int l = 0; l < levels; ++l) {
    const uint32_t nblk = 1u << l, B = P >> l, lgB = 31u - (uint32_t)__clz((int)B);
    float *cc = L.cell + (size_t)cur * half * 12, *cn = L.cell + (size_t)(cur ^ 1) * half * 12;
    for (uint32_t s = tid; s < nblk; s += kKdNT) {
      int dim = 0;
      float wd = -1.f;
      for (int d = 0; d < 6; ++d) {
        const float w = cc[s * 12 + 6 + d] - cc[s * 12 + d];
        if (w > wd) wd = w, dim = d;
      }
      L.sdim[s] = dim;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const uint32_t pos = (uint32_t)e * kKdNT + (uint32_t)tid, blk = pos >> lgB, r = pos & (B - 1u);
      const uint32_t cnt = seg_lo(n, l, blk + 1u) - seg_lo(n, l, blk);
      const uint32_t slot = (uint32_t)key[e];
      key[e] = r < cnt ? (((unsigned long long)f2ord(L.sf[slot][L.sdim[blk]]) << 32) | slot) : kKdPadKey;
    }
    kd_block_sort<E, kKdNT>(key, tid, B, L.xbuf);
#pragma unroll
    for (int e = 0; e < E; ++e) L.xbuf[e * kKdNT + tid] = key[e];
    __syncthreads();
    for (uint32_t s = tid; s < nblk; s += kKdNT) {
      const uint32_t a = seg_lo(n, l, s), b = seg_lo(n, l, s + 1u), nl = seg_lo(n, l + 1, 2u * s + 1u) - a;
      const int dim = L.sdim[s];
      float v = 0.5f * (cc[s * 12 + dim] + cc[s * 12 + 6 + dim]);
      if (b > a) v = L.sf[(uint32_t)L.xbuf[s * B + min(nl, b - a - 1u)]][dim];
      if (kPlanes) {
        const uint32_t h = (heap0 << l) + s;
        plane_dim[h] = dim;
        plane_val[h] = (double)v;
      }
      if (l + 1 < levels)
        for (int d = 0; d < 12; ++d) {
          const float c = cc[s * 12 + d];
          cn[(2u * s) * 12 + d] = (d == 6 + dim) ? v : c;
          cn[(2u * s + 1u) * 12 + d] = (d == dim) ? v : c;
        }
    }
    // the upper half of a block's elements to the front of its upper half
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const uint32_t pos = (uint32_t)e * kKdNT + (uint32_t)tid, blk = pos >> lgB, r = pos & (B - 1u), hb = B >> 1;
      const uint32_t a = seg_lo(n, l, blk), cnt = seg_lo(n, l, blk + 1u) - a, nl = seg_lo(n, l + 1, 2u * blk + 1u) - a;
      if (r < hb)
        key[e] = r < nl ? key[e] : kKdPadKey;
      else
        key[e] = (r - hb) < (cnt - nl) ? L.xbuf[blk * B + nl + (r - hb)] : kKdPadKey;
    }
    __syncthreads();
    cur ^= 1;
  }
#pragma unroll
  for (int e = 0; e < E; ++e) L.xbuf[e * kKdNT + tid] = key[e];
  __syncthreads();
}

__device__ __forceinline__ uint32_t kd_mix(uint32_t x) {  // (murmur3's finaliser: the sample must not beat against the order of the targets)
  x ^= x >> 16, x *= 0x85EBCA6Bu, x ^= x >> 13, x *= 0xC2B2AE35u, x ^= x >> 16;
  return x;
}

// ---- top stage: the planes of `ts` levels below every node of depth `depth0`, from a sample of the node's points ------------------
__global__ void __launch_bounds__(kKdTopNT) k_kd_top(const double *__restrict__ feat, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ starts,
                                                    uint32_t n, int depth0, int ts, int *plane_dim, double *plane_val, uint32_t *count) {
  constexpr int kKdNT = kKdTopNT, E = kKdSample / kKdNT;
  // the counters of this node's 2^ts buckets (k_kd_route adds to them next): cleared here instead of by a memset between the launches
  if ((int)threadIdx.x < (1 << ts)) count[(((size_t)blockIdx.x << ts) + threadIdx.x) * kKdPad] = 0u;
  __shared__ float s_sf[kKdSample][6];
  __shared__ unsigned long long s_x[2 * kKdSample];
  __shared__ float s_cell[2 * (1 << (kKdStageMax - 1)) * 12];
  __shared__ int s_dim[1 << (kKdStageMax - 1)];
  __shared__ uint32_t s_box[12];
  const int tid = threadIdx.x;
  const uint32_t parent = blockIdx.x;
  const uint32_t a = starts ? starts[parent] : 0u, b = starts ? starts[parent + 1] : n, nb = b - a;
  static_assert(E == 1, "one sample per thread");
  __shared__ uint32_t s_samp[kKdSample];
  __shared__ uint32_t s_cnt;
  KdLds L{s_sf, s_x, s_cell, s_dim, s_box};
  unsigned long long key[E];
  uint32_t cnt;
  if (!idx) {  // the first stage: one point out of every stratum of n / 1024 points of the call's order, at a hashed place inside it
    // (the plain stride - every (n / 1024)-th point - beat against the order of a window whose sweeps list the same surfaces in the
    // same order: the odometry step's 250 k-surfel window came out with buckets of up to 1 631 points for an average of 488)
    cnt = min((uint32_t)kKdSample, nb);
    const uint32_t lo = (uint32_t)(((uint64_t)tid * nb) / cnt), hi = (uint32_t)(((uint64_t)(tid + 1) * nb) / cnt);
    key[0] = (uint32_t)tid < cnt ? (unsigned long long)(a + lo + (hi > lo ? kd_mix((uint32_t)tid) % (hi - lo) : 0u)) : kKdPadKey;
  } else {
    // A later stage samples a node's points out of the scattered list, whose order inside a node is whatever the atomics made it.
    // The SAMPLE must not depend on that order - two calls (or two ranks of a query-sharded search) have to build the same tree -,
    // so it is defined by the points themselves: those whose HASHED target index is a multiple of m (m = points / 768, doubled in
    // the rare case that more than 1 024 qualify), put into ascending order.  (The first version took every k-th entry of
    // the list: planes, and with them bucket sizes, changed from call to call; a C4 window's tree came out with buckets beyond
    // 2 048 points in half of the calls - 2.6 ms in the in-place path of k_kd_bottom.)
    for (uint32_t m = max(1u, nb / 768u);; m *= 2u) {
      if (tid == 0) s_cnt = 0u;
      __syncthreads();
      for (uint32_t pos = a + (uint32_t)tid; pos < b; pos += kKdNT) {
        const uint32_t o = idx[pos];
        if (kd_mix(o) % m == 0u) {
          const uint32_t k = atomicAdd(&s_cnt, 1u);
          if (k < (uint32_t)kKdSample) s_samp[k] = o;
        }
      }
      __syncthreads();
      cnt = s_cnt;
      __syncthreads();
      if (cnt <= (uint32_t)kKdSample) break;
    }
    key[0] = (uint32_t)tid < cnt ? (unsigned long long)s_samp[tid] : kKdPadKey;
    kd_block_sort<E, kKdNT>(key, tid, (uint32_t)kKdSample, L.xbuf);
  }
  if ((uint32_t)tid < cnt) {
    const uint32_t o = (uint32_t)key[0];
    for (int d = 0; d < 6; ++d) s_sf[tid][d] = (float)feat[(size_t)o * 6 + d];
    key[0] = (unsigned long long)tid;
  }
  __syncthreads();
  kd_root_cell<E, kKdNT>(L, cnt, tid);
  kd_sort_levels<E, kKdNT, true>(key, L, cnt, ts, tid, (1u << depth0) + parent, plane_dim, plane_val);
}

// ---- every point through the planes of the first T levels -> its bucket; bucket sizes (LDS-aggregated, one counter per line) -----
__global__ void __launch_bounds__(1024) k_kd_route(const double *__restrict__ feat, uint32_t n, int T, const int *__restrict__ plane_dim,
                                                  const double *__restrict__ plane_val, uint32_t *bucket, uint32_t *count) {
  __shared__ uint32_t s_hist[1 << kKdTMax];
  const uint32_t nbk = 1u << T;
  for (uint32_t e = threadIdx.x; e < nbk; e += blockDim.x) s_hist[e] = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    uint32_t b = 0;
    for (int d = 0; d < T; ++d) {
      const uint32_t h = (1u << d) + b;
      b = 2u * b + (feat[(size_t)i * 6 + plane_dim[h]] >= plane_val[h] ? 1u : 0u);
    }
    bucket[i] = b;
    atomicAdd(&s_hist[b], 1u);
  }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < nbk; e += blockDim.x) {
    const uint32_t c = s_hist[e];
    if (c) atomicAdd(&count[(size_t)e * kKdPad], c);
  }
}

// starts[b] = points in buckets < b; the counters become the scatter's cursors
__global__ void __launch_bounds__(1024) k_kd_scan(uint32_t *count, uint32_t nbk, uint32_t *starts) {
  __shared__ uint32_t s_part[1024];
  const uint32_t per = (nbk + 1023u) / 1024u, lo = threadIdx.x * per, hi = min(nbk, lo + per);
  uint32_t sum = 0;
  for (uint32_t e = lo; e < hi; ++e) sum += count[(size_t)e * kKdPad];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const uint32_t v = threadIdx.x >= (unsigned)off ? s_part[threadIdx.x - off] : 0u;
    __syncthreads();
    s_part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = s_part[threadIdx.x] - sum;
  for (uint32_t e = lo; e < hi; ++e) {
    const uint32_t c = count[(size_t)e * kKdPad];
    starts[e] = run;
    count[(size_t)e * kKdPad] = run;
    run += c;
  }
  if (threadIdx.x == 1023) starts[nbk] = s_part[1023];
}

// bucket-wise scatter of the point indices (order inside a bucket: whatever the atomics make it - k_kd_bottom sorts it)
__global__ void __launch_bounds__(1024) k_kd_scatter(const uint32_t *__restrict__ bucket, uint32_t n, int T, uint32_t *cursor, uint32_t *idx_out) {
  __shared__ uint32_t s_hist[1 << kKdTMax];
  const uint32_t nbk = 1u << T;
  for (uint32_t e = threadIdx.x; e < nbk; e += blockDim.x) s_hist[e] = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t b = 0, r = 0;
  if (i < n) {
    b = bucket[i];
    r = atomicAdd(&s_hist[b], 1u);
  }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < nbk; e += blockDim.x) {
    const uint32_t c = s_hist[e];
    if (c) s_hist[e] = atomicAdd(&cursor[(size_t)e * kKdPad], c);
  }
  __syncthreads();
  if (i < n) idx_out[s_hist[b] + r] = i;
}

// ---- bottom: one workgroup per bucket ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void kd_box_store(float4 *box, uint32_t h, const float *b12) {
  box[(size_t)h * 3 + 0] = make_float4(b12[0], b12[1], b12[2], b12[3]);
  box[(size_t)h * 3 + 1] = make_float4(b12[4], b12[5], b12[6], b12[7]);
  box[(size_t)h * 3 + 2] = make_float4(b12[8], b12[9], b12[10], b12[11]);
}

struct KdOut {
  float4 *box;
  uint32_t *leaf_begin;
  float4 *pts32;  // 2 x float4 per sorted target: f0..f3 | f4 f5 <target index> 0 (the in-place path reads them back for its leaf boxes)
  double *sfeat;
  uint32_t *sorig;
};

// a bucket of nb <= E x 256 points: canonical order (ascending target index), the kd levels, the sorted copies, the leaf boxes
template <int E, int kKdNT>
__device__ void kd_bucket(const double *__restrict__ feat, const uint32_t *idx, uint32_t a, uint32_t nb, int Bd, const KdLds &L, uint32_t *s_orig,
                          float *s_boxes, const KdOut &O, int tid) {
  constexpr uint32_t P = (uint32_t)E * kKdNT;
  unsigned long long key[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t s = (uint32_t)e * kKdNT + (uint32_t)tid;
    key[e] = s < nb ? (unsigned long long)(idx ? idx[a + s] : a + s) : kKdPadKey;
  }
  if (idx) kd_block_sort<E, kKdNT>(key, tid, P, L.xbuf);  // (the scatter's order inside a bucket is not reproducible)
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t s = (uint32_t)e * kKdNT + (uint32_t)tid;
    if (s < nb) {
      const uint32_t o = (uint32_t)key[e];
      s_orig[s] = o;
      for (int d = 0; d < 6; ++d) L.sf[s][d] = (float)feat[(size_t)o * 6 + d];
      key[e] = s;
    }
  }
  __syncthreads();
  kd_root_cell<E, kKdNT>(L, nb, tid);
  kd_sort_levels<E, kKdNT, false>(key, L, nb, Bd, tid, 0u, nullptr, nullptr);
  // sorted copies: leaf i = block i of P >> Bd keys, its points behind a + seg_lo(nb, Bd, i)
  const uint32_t Bf = P >> Bd, lgBf = 31u - (uint32_t)__clz((int)Bf), nleaf = 1u << Bd;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t pos = (uint32_t)e * kKdNT + (uint32_t)tid, leaf = pos >> lgBf, r = pos & (Bf - 1u);
    const uint32_t la = seg_lo(nb, Bd, leaf), cnt = seg_lo(nb, Bd, leaf + 1u) - la;
    if (r < cnt) {
      const uint32_t slot = (uint32_t)key[e], o = s_orig[slot];
      const size_t g = (size_t)a + la + r;
      O.sorig[g] = o;
      O.pts32[g * 2 + 0] = make_float4(L.sf[slot][0], L.sf[slot][1], L.sf[slot][2], L.sf[slot][3]);
      O.pts32[g * 2 + 1] = make_float4(L.sf[slot][4], L.sf[slot][5], __uint_as_float(o), 0.f);
      for (int d = 0; d < 6; ++d) O.sfeat[g * 6 + d] = feat[(size_t)o * 6 + d];
    }
  }
  for (uint32_t i = tid; i < nleaf; i += kKdNT) {
    const uint32_t cnt = seg_lo(nb, Bd, i + 1u) - seg_lo(nb, Bd, i);
    float bx[12];
    for (int d = 0; d < 6; ++d) bx[d] = 3.0e38f, bx[6 + d] = -3.0e38f;
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint32_t slot = (uint32_t)L.xbuf[i * Bf + r];
      for (int d = 0; d < 6; ++d) bx[d] = fminf(bx[d], L.sf[slot][d]), bx[6 + d] = fmaxf(bx[6 + d], L.sf[slot][d]);
    }
    for (int d = 0; d < 12; ++d) s_boxes[(size_t)(nleaf + i) * 12 + d] = bx[d];
  }
}

// kCap = 1024: the buckets of up to 1024 points (nearly all: an average bucket holds 256 - 512), 50 KB of LDS, three workgroups
// per CU.  kCap = 2048: a second launch for the larger ones; what does not fit there either (many coincident features, or more
// than 4 M targets) gets no kd order below the bucket: its indices are sorted in place in global memory (canonical order), the
// leaves are even pieces of that order.
template <int kCap>
__global__ void __launch_bounds__(kKdBotNT) k_kd_bottom(const double *__restrict__ feat, uint32_t *idx, const uint32_t *__restrict__ starts, uint32_t n, int T,
                                                    int Bd, KdOut O) {
  __shared__ float s_sf[kCap][6];
  __shared__ unsigned long long s_x[2 * kCap];
  __shared__ uint32_t s_orig[kCap];
  __shared__ float s_cell[2 * (1 << (kKdBdMax - 1)) * 12];
  __shared__ int s_dim[1 << (kKdBdMax - 1)];
  __shared__ float s_boxes[(2 << kKdBdMax) * 12];  // the bucket's subtree, local heap order
  __shared__ uint32_t s_box[12];
  constexpr int kKdNT = kKdBotNT;
  const int tid = threadIdx.x, nthr = kKdNT;
  const uint32_t bk = blockIdx.x;
  const uint32_t a = starts ? starts[bk] : 0u, b = starts ? starts[bk + 1] : n, nb = b - a;
  if (kCap == 1024 ? nb > 1024u : nb <= 1024u) return;  // (the other launch's bucket)
  const uint32_t nleaf = 1u << Bd;
  for (uint32_t i = tid; i < nleaf; i += nthr) O.leaf_begin[((size_t)bk << Bd) + i] = a + seg_lo(nb, Bd, i);
  if (bk + 1u == (1u << T) && tid == 0) O.leaf_begin[(size_t)1 << (T + Bd)] = n;
  KdLds L{s_sf, s_x, s_cell, s_dim, s_box};
  if (kCap == 1024) {
    if (nb <= 512u)
      kd_bucket<1, kKdNT>(feat, idx, a, nb, Bd, L, s_orig, s_boxes, O, tid);
    else
      kd_bucket<2, kKdNT>(feat, idx, a, nb, Bd, L, s_orig, s_boxes, O, tid);
  } else if (nb <= 2048u) {
    kd_bucket<(kCap == 1024 ? 2 : 4), kKdNT>(feat, idx, a, nb, Bd, L, s_orig, s_boxes, O, tid);
  } else {
    for (uint32_t k = 2; (k >> 1) < nb; k <<= 1) {  // (normalised network: any length sorts)
      bool first = true;
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        const uint32_t mask = first ? (k - 1u) : j;
        for (uint32_t r = tid; r < nb; r += nthr) {
          const uint32_t pr = r ^ mask;
          if (pr > r && pr < nb) {
            const uint32_t x = idx[a + r], y = idx[a + pr];
            if (y < x) idx[a + r] = y, idx[a + pr] = x;
          }
        }
        first = false;
        __syncthreads();
      }
    }
    for (uint32_t pos = tid; pos < nb; pos += nthr) {
      const uint32_t o = idx[a + pos];
      float f32[6];
      for (int d = 0; d < 6; ++d) {
        const double v = feat[(size_t)o * 6 + d];
        O.sfeat[(size_t)(a + pos) * 6 + d] = v;
        f32[d] = (float)v;
      }
      O.sorig[a + pos] = o;
      O.pts32[(size_t)(a + pos) * 2 + 0] = make_float4(f32[0], f32[1], f32[2], f32[3]);
      O.pts32[(size_t)(a + pos) * 2 + 1] = make_float4(f32[4], f32[5], __uint_as_float(o), 0.f);
    }
    __syncthreads();  // (the stores above are read back below by other threads of this workgroup)
    for (uint32_t i = tid; i < nleaf; i += nthr) {
      const uint32_t la = seg_lo(nb, Bd, i), lb = seg_lo(nb, Bd, i + 1u);
      float bx[12];
      for (int d = 0; d < 6; ++d) bx[d] = 3.0e38f, bx[6 + d] = -3.0e38f;
      for (uint32_t p = la; p < lb; ++p) {
        const float4 p0 = O.pts32[(size_t)(a + p) * 2], p1 = O.pts32[(size_t)(a + p) * 2 + 1];
        const float f32[6] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y};
        for (int d = 0; d < 6; ++d) bx[d] = fminf(bx[d], f32[d]), bx[6 + d] = fmaxf(bx[6 + d], f32[d]);
      }
      for (int d = 0; d < 12; ++d) s_boxes[(size_t)(nleaf + i) * 12 + d] = bx[d];
    }
  }
  __syncthreads();
  // the bucket's subtree bottom-up (local heap: node (j, i) = (1 << j) + i), then out to the global heap at depth T + j
  for (int j = Bd - 1; j >= 0; --j) {
    for (uint32_t i = tid; i < (1u << j); i += nthr) {
      const uint32_t h = (1u << j) + i;
      for (int d = 0; d < 6; ++d) {
        s_boxes[(size_t)h * 12 + d] = fminf(s_boxes[(size_t)(2 * h) * 12 + d], s_boxes[(size_t)(2 * h + 1) * 12 + d]);
        s_boxes[(size_t)h * 12 + 6 + d] = fmaxf(s_boxes[(size_t)(2 * h) * 12 + 6 + d], s_boxes[(size_t)(2 * h + 1) * 12 + 6 + d]);
      }
    }
    __syncthreads();
  }
  for (uint32_t h = 1u + tid; h < (2u << Bd); h += nthr) {
    const int j = 31 - __clz((int)h);
    const uint32_t i = h - (1u << j);
    kd_box_store(O.box, (1u << (T + j)) + (bk << j) + i, &s_boxes[(size_t)h * 12]);
  }
}

// the levels above the buckets, bottom-up (one workgroup; global stores of a level are read by the next behind a barrier)
__global__ void __launch_bounds__(1024) k_kd_top_boxes(float4 *box, int T) {
  for (int d = T - 1; d >= 0; --d) {
    for (uint32_t i = threadIdx.x; i < (1u << d); i += blockDim.x) {
      const uint32_t h = (1u << d) + i;
      const float4 a0 = box[(size_t)(2 * h) * 3], a1 = box[(size_t)(2 * h) * 3 + 1], a2 = box[(size_t)(2 * h) * 3 + 2];
      const float4 b0 = box[(size_t)(2 * h + 1) * 3], b1 = box[(size_t)(2 * h + 1) * 3 + 1], b2 = box[(size_t)(2 * h + 1) * 3 + 2];
      box[(size_t)h * 3 + 0] = make_float4(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z), fminf(a0.w, b0.w));
      box[(size_t)h * 3 + 1] = make_float4(fminf(a1.x, b1.x), fminf(a1.y, b1.y), fmaxf(a1.z, b1.z), fmaxf(a1.w, b1.w));
      box[(size_t)h * 3 + 2] = make_float4(fmaxf(a2.x, b2.x), fmaxf(a2.y, b2.y), fmaxf(a2.z, b2.z), fmaxf(a2.w, b2.w));
    }
    __threadfence_block();
    __syncthreads();
  }
}

// ---- traversal --------------------------------------------------------------------------------------------------------------------
// squared distance of the (fp32) query to a box, 0 inside; empty boxes (lo0 > hi0) are reported separately
__device__ __forceinline__ float kd_box_d2(const float4 b0, const float4 b1, const float4 b2, const float *qf) {
  const float d0 = fmaxf(fmaxf(b0.x - qf[0], qf[0] - b1.z), 0.f), d1 = fmaxf(fmaxf(b0.y - qf[1], qf[1] - b1.w), 0.f);
  const float d2 = fmaxf(fmaxf(b0.z - qf[2], qf[2] - b2.x), 0.f), d3 = fmaxf(fmaxf(b0.w - qf[3], qf[3] - b2.y), 0.f);
  const float d4 = fmaxf(fmaxf(b1.x - qf[4], qf[4] - b2.z), 0.f), d5 = fmaxf(fmaxf(b1.y - qf[5], qf[5] - b2.w), 0.f);
  return d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3 + d4 * d4 + d5 * d5;
}

// exact k-NN + gates through the tree, EIGHT LANES PER QUERY: a depth-first walk, nearest box first, pruned against the k-th
// distance in all six dimensions.  The group's lane j takes child j of a node (three levels per step: the 8 boxes are 384 contiguous
// bytes, 48 per lane) or point j of a leaf (its fp64 feature, 48 bytes per lane, summed exactly at once: a fp32 first look would be a
// second dependent round trip for whoever passes), the survivors are ranked inside the group, the k best live in the group's registers
// (two entries per lane) and the pending work is ONE stack per group in LDS (nodes and leaves alike, farthest pushed first): every
// round trip is one coalesced load, a wavefront is eight independent walks, and eight times as many wavefronts hide each other's
// latency.  (Rounds 4 - 5 also had a walk of ONE lane per query: a search of 40 k queries is 630 of its
// wavefronts on a chip with 4 096 slots, and it lasted as long as ONE wavefront's chain of ~80 steps of up to ten dependent round
// trips - 0.9 ms of the room stream's 1.12 ms search.  That walk and the other shapes that were built and measured: DESIGN 3.3.)
// It is VALU-bound (87 % busy on the odometry step's fixed-window search): ~260 vector
// instructions per round of a wavefront, in which each of its eight groups takes ONE item - so both the node and the leaf code run
// in nearly every round.  What the round costs was found in the ISA (llvm-objdump): a sorted list was ~125 instructions and twelve
// ds_bpermute per insertion - now unsorted, the k-th entry looked for again after an insertion (find_worst: ~25) and sorted once at
// the end -; the ranking of the surviving children seven ds_bpermute - now DPP moves; node / leaf nested under `if (sp > 0)` ~45 register
// copies of the list per round - now two flat branches behind an unconditional pop.  250 k queries against 62 k targets: 1.45 ->
// 1.23 ms, the same set 1.08 -> 0.94.  Not kept: one 8-point chunk per round with the leaf's rest pushed back and the insertions at
// the top level of the round (more instructions, not fewer copies); a wave-uniform insertion loop (86 copies instead of 55); a pop
// that skips, in a loop of its own, the entries the k-th distance has overtaken since they were pushed (20 - 27 of a query's ~60 pops:
// the rounds of a wavefront per query 67 -> 41 and 80 -> 62, the time unchanged - such a round was cheap already, the branches of a
// group that has nothing to do are skipped when no other group takes them); ONE kind of item per round, the kind most of the
// wavefront's groups have on top, the others waiting (0.98 / 1.23 against 0.96 / 1.24 ms: the rounds get cheaper and more).
// Exact: the order (distance, index) is total, so the list does not depend on the order in which the walk meets the targets.
// stats (sampled: one wavefront in 64): [0] nodes opened, [1] leaves scanned, [2] points looked at, [3] exact distances, [4] queries
// Round 5, built, measured and taken out again - a REFILLING launch: one wavefront per slot of the chip (6 144), a group whose walk has
// ended stores its list as it stands (a second kernel, one lane per query, sorts and gates: 50 - 69 us at 250 k queries) and takes the
// next place of the walk order from the wavefront's range, the wavefront chunks of 8 - 64 places from one counter; the features by place
// (the tree's sorted copy) so that a refill is one round trip.  Same pairs byte for byte - and the walk kernel of the step-like window
// 475 -> 708 us (same set) and 808 -> 1 095 us (fixed window), C4's searches 1.86 -> 2.8 and 3.5 -> 4.8 ms, whatever the chunk (guided
// chunks, 68 k atomics, were no different from 31 k of eight) and with half the wavefronts only 1.35 x slower still.  Why: the eight
// queries of a plain wavefront are neighbours in leaf order that START TOGETHER - they descend through the same nodes and reach their
// leaves in the same rounds, so most rounds of the wavefront run ONE of the two branches (node / leaf); groups that refill at
// different times are out of step and nearly every round runs both (~2 x the instructions per round against the ~1.3 x a wavefront
// loses waiting for the slowest of its eight walks).  What balances a launch is its ~5 rounds of wavefronts, handed out by the
// hardware as slots come free.
// A stack entry: x = squared distance (fp32 bits; a leaf keeps its point count - 1 in the low 5 bits: rounded towards zero, which
// is conservative), y = heap index of a node, or 1 << 31 | first point of a leaf (1 << 30 set: the leaf's index instead - more
// than 32 points, its range is looked up).
template <int CTRL>
__device__ __forceinline__ uint32_t kd_dpp(uint32_t v) {  // v of another lane of the row (DPP control CTRL), as a VALU move
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double kd_dpp_f64(double v) {
  return __hiloint2double((int)kd_dpp<CTRL>((uint32_t)__double2hiint(v)), (int)kd_dpp<CTRL>((uint32_t)__double2loint(v)));
}
constexpr int kGroupStack = 52;  // 1 + 7 per 3-level step, D <= 21
// EARLY (round 6, a search against ANOTHER set whose neighbour lists nobody asked for): the reference takes the FIRST of the k neighbours
// that passes the gates (knn_surfel_matcher.cc:24-46; with two different sets no pair can have been seen before, cc:35-38), so what a
// query needs is its nearest gate-passing target a - and the targets in front of a, to know whether a is among the k nearest.  The
// walk's bound is min(k-th entry, nearest candidate ACCEPTED so far): accepted = passes the three gates with a margin, judged from
// what the lane holds anyway (the two features: centre difference and normals to ~1e-15, the margins are 1e-9) + the target's stamp.
// Sound because an accepted candidate really passes (the exact gates still run on the final list, from the world-frame copies): every
// target in front of the nearest accepted one is visited under the plain k-NN rule, so the list's part in front of it is exact and the
// first entry that passes the exact gates is the reference's choice; entries behind it are whatever the walk met.  Only the FIRST
// entry of the gated list is meaningful in this mode (k_resolve reads no other for two sets).
// ONE set (the sliding-window search): k_resolve skips a candidate c of query q only when c < q (and c chose q, cc:35-38) - a candidate
// with c > q always ends the scan of q's list.  There the accepted candidates are the gate-passing ones with c > q: the list is exact
// up to the nearest of them, and the resolve rounds never read beyond it.
template <int K, int NT, bool EARLY>
// (six wavefronts per SIMD: 80 registers, two spills outside the walk - the feature and the gates hold the peak -; five without the bound.
// 250 k queries: 0.96 / 1.24 -> 0.89 / 1.16 ms; seven or eight wavefronts - 8 / 9 spills - no better)
// NT = threads per workgroup (NT / 8 queries): the groups of a workgroup share nothing but the launch; launched with NT = 64 (match.hip)
// (Measured, not kept: an XCD-aware hand-out - workgroup b takes block (b mod 8) * n / 8 + b / 8 of the leaf order, so that an XCD's L2
// serves one eighth of the tree - 1.614 -> 1.65 ms for the step-like pair, 1.12 -> 1.165 for its fixed-window search: the walks are
// VALU-bound, and eighths of the order differ in cost, so seven XCDs wait for the one with the hard region.)
__global__ void __launch_bounds__(NT, 6) k_knn_tree_group(const wc_surfel *q_surf, const wc_pose *q_pose, uint32_t nq, KdTree T, int first3, const double *tworld,
                                                       uint32_t nt, MatchParams M, uint32_t *gated, uint32_t *knn_idx, double *knn_d2,
                                                       const uint32_t *__restrict__ qorder, uint32_t q_begin, uint32_t q_end, uint32_t *gated_shard,
                                                       unsigned long long *stats, uint32_t *status) {
  static_assert(K <= 16, "two list entries per lane");
  __shared__ uint2 s_stack[NT / 8][kGroupStack];
  const int lane = threadIdx.x & 63, sub = lane & 7, gbase = lane & ~7, grp = threadIdx.x >> 3;
  const uint32_t qi = q_begin + blockIdx.x * (uint32_t)(NT / 8) + (uint32_t)grp;
  const bool live = qi < q_end;
  const uint32_t q = live ? (qorder ? qorder[qi] : qi) : 0u;
  double f[6];
  {
    V3 cq0, nq0;  // (what the gates need of the query - centre, normal, stamp - is formed again behind the walk: 14 registers less in it)
    feature6(q_surf[q], q_pose[q], M.cs, M.as, f, cq0, nq0);
  }
  float qf[6];
  double qmax = 0.0;
#pragma unroll
  for (int d = 0; d < 6; ++d) qf[d] = (float)f[d], qmax = fmax(qmax, fabs(f[d]));
  // the list: entry e = sub + 8 * slot, UNSORTED while the walk lasts (a new entry takes the place of the k-th = the largest by
  // (distance, index), which is then looked for again: three exchange steps inside the group, as DPP moves); sorted once at the
  // end.  Keeping it sorted cost ~125 instructions per insertion - twelve ds_bpermute among them -, this ~60.  Empty = (-1, 0):
  // never the largest.
  double ld0 = -1.0, ld1 = -1.0;
  uint32_t li0 = 0u, li1 = 0u;
  int have = 0;  // (uniform in the group)
  double ld_worst = 1e300;  // the k-th entry (uniform in the group); meaningful when have == K
  uint32_t li_worst = 0xFFFFFFFFu;
  auto gbyte = [&](bool p) -> uint32_t { return (uint32_t)(__ballot(p) >> gbase) & 0xFFu; };
  auto find_worst = [&]() {
    // the largest distance first (v_max_f64 behind DPP moves), then the largest index among the entries that have it: a compare of
    // (distance, index) pairs per step was twice the instructions, and two entries at the same distance are the exception
    double d = sub + 8 < K ? fmax(ld0, ld1) : ld0;
    d = fmax(d, kd_dpp_f64<0xB1>(d));   // lane ^ 1
    d = fmax(d, kd_dpp_f64<0x4E>(d));   // lane ^ 2
    d = fmax(d, kd_dpp_f64<0x141>(d));  // lane -> 7 - lane: the other quad
    uint32_t i = ld0 == d ? li0 : 0u;
    if (sub + 8 < K) i = max(i, ld1 == d ? li1 : 0u);
    i = max(i, kd_dpp<0xB1>(i));
    i = max(i, kd_dpp<0x4E>(i));
    i = max(i, kd_dpp<0x141>(i));
    ld_worst = d, li_worst = i;
  };
  // The look at a box is taken in fp32 and only has to be conservative: whatever passes is summed exactly, in fp64 and in
  // flann::L2_Simple's order.  A target the walk still needs has |d_i| <= sqrt(w) in every component (w = the walk's bound), so its
  // components are at most qmax + sqrt(w) in magnitude; a box bound is the fp32 image of a target coordinate, and the fp32 images of
  // query and bound are off by 2^-24 of their magnitudes: a difference by delta = 2^-23 (2 qmax + sqrt(w)) including its own
  // rounding, a square by 2 sqrt(w) delta + delta^2, the six-term fp32 sum by a few 2^-24 of itself.  (sqrt(w) is bounded by
  // (w + 1) / 2.)
  auto thr32_of = [&](double w) -> float {
    if (!(w < 1e30)) return __builtin_inff();
    const double sw = 0.5 * (w + 1.0), delta = 1.1920928955078125e-7 * (2.0 * qmax + sw) * 1.01;
    return __double2float_ru(w * (1.0 + 4e-6) + 6.2 * (2.0 * sw * delta + delta * delta) + 1e-30);
  };
  float thr32 = __builtin_inff();
  // the walk's bound (uniform in the group): the k-th entry of a full list; EARLY: or the nearest accepted candidate (ad, ai)
  double bd = 1e300, ad = 1e300;
  uint32_t bi = 0xFFFFFFFFu, ai = 0xFFFFFFFFu;
  const double tq_e = EARLY ? q_surf[q].t : 0.0;
  uint32_t st_nodes = 0, st_leaves = 0, st_pts = 0, st_exact = 0;
  int sp = 0;
  if (live) {
    if (sub == 0) s_stack[grp][0] = T.D == 0 ? make_uint2(0u, 0xC0000000u) : make_uint2(0u, 1u);  // leaf 0 (range looked up) / the root
    sp = 1;
  }
  __builtin_amdgcn_wave_barrier();
  while (__any(sp > 0)) {
    {
      // (two flat branches - node, leaf - behind one unconditional pop: nested as if / else inside `if (sp > 0)` the compiler carried
      // the list through ~45 register copies per round)
      const bool act = sp > 0;
      sp -= act ? 1 : 0;
      const uint2 en = s_stack[grp][sp];
      __builtin_amdgcn_wave_barrier();
      const bool is_leaf = (en.y >> 31) != 0u;
      const float d_en = __uint_as_float(is_leaf ? (en.x & ~31u) : en.x);
      const bool go = act & !(d_en > thr32);
      {
        if (go & !is_leaf) {
          // ---- a node: lane j looks at child j (the box, and for a leaf child its point range, in one round of loads)
          const uint32_t h = en.y;
          const int depth = 31 - __clz((int)h);
          const int ws = depth == 0 ? first3 : 3;
          const bool bottom = depth + ws == T.D;
          const uint32_t c = (h << ws) + (uint32_t)sub;
          const bool exists = sub < (1 << ws);
          ++st_nodes;
          float d2 = 0.f;
          bool ok = false;
          uint32_t lb = 0, le = 0;
          if (exists) {
            const float4 *bp = T.box + (size_t)c * 3;
            const float4 b0 = bp[0], b1 = bp[1], b2 = bp[2];
            if (bottom) lb = T.leaf_begin[c - (1u << T.D)], le = T.leaf_begin[c - (1u << T.D) + 1u];
            d2 = kd_box_d2(b0, b1, b2, qf);
            ok = !(b0.x > b1.z) && !(d2 > thr32) && (!bottom || le > lb);
          }
          // farthest first onto the stack: the nearest is popped next.  Rank among the survivors by (distance, child).
          const uint32_t key = ok ? ((__float_as_uint(d2) & ~7u) | (uint32_t)sub) : 0u;
          int above = 0;  // survivors farther than this one: the three others of the quad, then the other quad's four (DPP moves)
          {
            const uint32_t km = kd_dpp<0x141>(key);
            above += (kd_dpp<0xB1>(key) > key) + (kd_dpp<0x4E>(key) > key) + (kd_dpp<0x1B>(key) > key);
            above += (km > key) + (kd_dpp<0xB1>(km) > key) + (kd_dpp<0x4E>(km) > key) + (kd_dpp<0x1B>(km) > key);
          }
          const int nsurv = __popc(gbyte(ok));
          if (ok) {
            const int slot = sp + above;
            if (slot < kGroupStack) {
              uint2 e;
              if (bottom) {
                const uint32_t cnt = le - lb;
                if (cnt <= 32u)
                  e = make_uint2((__float_as_uint(d2) & ~31u) | (cnt - 1u), 0x80000000u | lb);
                else
                  e = make_uint2(__float_as_uint(d2) & ~31u, 0xC0000000u | (c - (1u << T.D)));
              } else {
                e = make_uint2(__float_as_uint(d2), c);
              }
              s_stack[grp][slot] = e;
            } else {
              atomicOr(&status[1], 8u);  // (cannot happen for D <= 21)
            }
          }
          sp = min(sp + nsurv, kGroupStack);
        }
        __builtin_amdgcn_wave_barrier();
        if (go & is_leaf) {
          // ---- a leaf: lane j looks at point j (fp32), the survivors are summed exactly and inserted one after the other
          uint32_t b, cnt;
          if (en.y & 0x40000000u) {
            const uint32_t leaf = en.y & 0x3FFFFFFFu;
            b = T.leaf_begin[leaf];
            cnt = T.leaf_begin[leaf + 1u] - b;
          } else {
            b = en.y & 0x3FFFFFFFu;
            cnt = (en.x & 31u) + 1u;
          }
          ++st_leaves;
          st_pts += cnt;
          for (uint32_t off = 0; off < cnt; off += 8u) {
            const bool has = off + (uint32_t)sub < cnt;
            const uint32_t i = b + off + (uint32_t)sub;
            // (the leaf's points straight in fp64 - 48 + 4 contiguous bytes per lane -: with one point per lane the fp32 first look
            // saves no arithmetic worth the name and costs a second, dependent round trip for whoever passes it)
            double s = 0.0;
            uint32_t id = 0xFFFFFFFFu;
            bool pass = false, acc = false;
            if (has) {
              const double *p = T.sfeat + (size_t)i * 6;
              id = T.sorig[i];
              double dn = 0.0, dp = 0.0;
#pragma unroll
              for (int d = 0; d < 6; ++d) {
                const double pv = p[d], df = f[d] - pv;
                s += df * df;
                if (EARLY && d >= 3) dn += f[d] * pv;
                if (EARLY && d < 3) dp += f[d + 3] * df;
              }
              ++st_exact;
              pass = !(s > bd);
              if (EARLY) {
                // cos of the angle between the normals / distance along the query's normal, to ~1e-15 of the gates' own operands
                acc = pass && dn * M.as * M.as >= M.cos_acc && fabs(dp) * M.as * M.cs <= M.plane_acc - 1e-9 * qmax * M.cs && (!M.same_set || id > q);
                if (acc) acc = !(fabs(tworld[(size_t)id * 7 + 6] - tq_e) < M.time_min);
              }
            }
            uint32_t pm = gbyte(pass);
            const uint32_t am = EARLY ? gbyte(acc) : 0u;
            bool inserted = false;
            // An EMPTY list takes the chunk's points as they stand - lane j's point becomes entry j -: the first leaf of a walk (all of
            // its up to eight points pass: there is no bound yet) was eight insertions one after the other, ~85 instructions each, a
            // quarter of a short walk's instructions.  (Uniform in the group; K >= 8: the entries fit.)
            if (K >= 8 && have == 0 && pm != 0u && (pm & (pm + 1u)) == 0u) {
              ld0 = pass ? s : ld0, li0 = pass ? id : li0;
              have = __popc(pm);
              inserted = true;
              if (have == K) find_worst();
              if (EARLY) {
                if (am) {  // the nearest accepted point of the chunk: smallest distance, then smallest index (DPP moves, as find_worst)
                  double d = acc ? s : 1e300;
                  d = fmin(d, kd_dpp_f64<0xB1>(d));
                  d = fmin(d, kd_dpp_f64<0x4E>(d));
                  d = fmin(d, kd_dpp_f64<0x141>(d));
                  uint32_t i = (acc && s == d) ? id : 0xFFFFFFFFu;
                  i = min(i, kd_dpp<0xB1>(i));
                  i = min(i, kd_dpp<0x4E>(i));
                  i = min(i, kd_dpp<0x141>(i));
                  ad = d, ai = i;
                }
                const bool wl = have == K && ((ld_worst < ad) | ((ld_worst == ad) & (li_worst < ai)));
                bd = wl ? ld_worst : ad, bi = wl ? li_worst : ai;
              } else if (have == K) {
                bd = ld_worst, bi = li_worst;
              }
              pm = 0u;
            }
            while (pm) {  // (wave-uniform - `while (__any(pm)) if (pm)` - compiles to more register copies, not fewer)
              const int src = __ffs((int)pm) - 1;
              pm &= pm - 1u;
              const double cs = __shfl(s, gbase + src);
              const uint32_t ci = (uint32_t)__shfl((int)id, gbase + src);
              // (one straight-line update: a full list gives up its k-th entry - (distance, index) is unique -, a list still filling
              // its next free place)
              const bool full = have == K;
              const bool reject = EARLY ? ((cs > bd) | ((cs == bd) & !(ci < bi))) : (full & ((cs > ld_worst) | ((cs == ld_worst) & !(ci < li_worst))));
              if (!reject) {
                const bool m0 = full ? ((ld0 == ld_worst) & (li0 == li_worst)) : (sub == have);
                const bool m1 = full ? ((ld1 == ld_worst) & (li1 == li_worst)) : (sub + 8 == have);
                ld0 = m0 ? cs : ld0, li0 = m0 ? ci : li0;
                ld1 = m1 ? cs : ld1, li1 = m1 ? ci : li1;
                have += full ? 0 : 1;
                inserted = true;
                if (have == K) find_worst();
                if (EARLY) {
                  if ((am >> src) & 1u) ad = cs, ai = ci;  // (not rejected: in front of the bound, so in front of the accepted one so far)
                  const bool wl = have == K && ((ld_worst < ad) | ((ld_worst == ad) & (li_worst < ai)));
                  bd = wl ? ld_worst : ad, bi = wl ? li_worst : ai;
                } else if (have == K) {
                  bd = ld_worst, bi = li_worst;
                }
              }
            }
            if (inserted && bd < 1e299) thr32 = thr32_of(bd);
          }
        }
      }
    }
  }
  if (stats && (blockIdx.x & 63u) == 0u) {
    unsigned long long v[5] = {sub == 0 ? st_nodes : 0u, sub == 0 ? st_leaves : 0u, sub == 0 ? st_pts : 0u, st_exact, (live && sub == 0) ? 1ull : 0ull};
    for (int j = 0; j < 5; ++j) {
      for (int m = 1; m < 64; m <<= 1) v[j] += __shfl_xor(v[j], m);
      if (lane == 0) atomicAdd(&stats[j], v[j]);
    }
  }
  // the list in neighbour order: every entry counts the entries in front of it (all of them pass through the group's - now empty -
  // stack in LDS) and moves to that place
  {
    double *sd = (double *)&s_stack[grp][0];
    uint32_t *si = (uint32_t *)&s_stack[grp][16];
    double *od = (double *)&s_stack[grp][24];
    uint32_t *oi = (uint32_t *)&s_stack[grp][40];
    static_assert(kGroupStack >= 48, "the sort's scratch");
    __builtin_amdgcn_wave_barrier();
    if (sub < have) sd[sub] = ld0, si[sub] = li0;
    if (sub + 8 < have) sd[sub + 8] = ld1, si[sub + 8] = li1;
    __builtin_amdgcn_wave_barrier();
    int r0 = 0, r1 = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if (t < have) {
        const double dt = sd[t];
        const uint32_t it = si[t];
        r0 += (dt < ld0 || (dt == ld0 && it < li0)) ? 1 : 0;
        r1 += (dt < ld1 || (dt == ld1 && it < li1)) ? 1 : 0;
      }
    }
    if (sub < have) od[r0] = ld0, oi[r0] = li0;
    if (sub + 8 < have) od[r1] = ld1, oi[r1] = li1;
    __builtin_amdgcn_wave_barrier();
    if (sub < have) ld0 = od[sub], li0 = oi[sub];
    if (sub + 8 < have) ld1 = od[sub + 8], li1 = oi[sub + 8];
  }
  // outputs: lane (e & 7), slot (e >> 3) holds neighbour e; Q10: FLANN leaves the tail of the result untouched (zero-initialised)
  // when fewer than k targets exist.  Gates cc:26 / cc:29 (surfel.h:105-107) / cc:32, the survivors in neighbour order.
  V3 cq, nq_w;
  {
    double f_again[6];
    feature6(q_surf[q], q_pose[q], M.cs, M.as, f_again, cq, nq_w);
  }
  const double tq = q_surf[q].t;
  bool pass[2];
  uint32_t cid[2];
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    const int e = sub + 8 * sl;
    const bool valid = live && e < K;
    const uint32_t c = (valid && e < have) ? (sl ? li1 : li0) : 0u;
    cid[sl] = c;
    pass[sl] = false;
    if (valid) {
      if (knn_idx) {
        knn_idx[(size_t)q * K + e] = c;
        knn_d2[(size_t)q * K + e] = e < have ? (sl ? ld1 : ld0) : 0.0;
      }
      const double *w = tworld + (size_t)c * 7;
      bool p = !(fabs(w[6] - tq) < M.time_min);
      const V3 nc = mk3(w[3], w[4], w[5]);
      const double dc = dot(nq_w, nc);
      p = p && !(dc < M.cos_min && dc >= -1.0);  // acos(dc) > ang_max as the HOST's acos decides it (match.hip: match_cos_gate); NaN passes
      p = p && !(fabs(dot(nq_w, cq - mk3(w[0], w[1], w[2]))) > M.dist_max);
      pass[sl] = p;
    }
  }
  const uint32_t pm0 = gbyte(pass[0]), pm1 = gbyte(pass[1]);
  const int npass = __popc(pm0) + __popc(pm1);
  // (two sets with the early bound, lists not gathered from other ranks: k_resolve reads a list's FIRST entry and no other - one
  // 4-byte store per query straight into plane 0, and the transposition of the lists behind the walk goes: C4's 1 M queries 113 us)
  // One set: the resolve rounds never read behind the accepted candidate that bounded the walk (a larger index: it always ends the
  // scan) - the planes are written up to its entry and no further, one to three scattered words per query instead of k.
  int o_stop = (EARLY && !M.same_set && !gated_shard) ? 0 : K;
  if (EARLY && M.same_set && !gated_shard && ai != 0xFFFFFFFFu) {
    const uint32_t m0 = gbyte(pass[0] && cid[0] == ai), m1 = gbyte(pass[1] && cid[1] == ai);
    if (m0)
      o_stop = __popc(pm0 & (m0 - 1u));
    else if (m1)
      o_stop = __popc(pm0) + __popc(pm1 & (m1 - 1u));
  }
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    const int e = sub + 8 * sl;
    if (!live || e >= K) continue;
    uint32_t *dst = gated_shard ? gated_shard + (size_t)(qi - q_begin) * K : nullptr;
    if (pass[sl]) {
      const int o = sl ? __popc(pm0) + __popc(pm1 & ((1u << sub) - 1u)) : __popc(pm0 & ((1u << sub) - 1u));
      if (dst)
        dst[o] = cid[sl];
      else if (o <= o_stop)
        gated[(size_t)o * nq + q] = cid[sl];
    }
    if (e >= npass) {
      if (dst)
        dst[e] = kNone;
      else if (e <= o_stop)
        gated[(size_t)e * nq + q] = kNone;
    }
  }
}
