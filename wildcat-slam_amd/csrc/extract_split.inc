// extract_split.inc — the node stage of the default extraction path as TWO kernels (included by extract.hip behind
// extract_fast.inc, whose tables, records and node-stage routines it uses).
//
// k_fx_nodes (extract_fast.inc) does everything that follows the streaming pass in one launch: it walks the record lists,
// finds the temporal clusters, tests the nodes (two PCAs per wavefront), emits, queues layer-2 nodes and cleans the tables.
// That is the right shape for ONE sweep of a million points - 488 wavefronts, less than one per SIMD, three launch heads
// per sweep - but the kernel needs 464 VGPRs: one wavefront per SIMD.  A 10 M-point cloud (or ten sweeps enqueued together)
// has ~5 000 of them, five rounds at 5 % occupancy, and the knock-out runs (profiles/exp_knockout.sh, 10 M points) put 72 of
// its 126 us into the node tests + emission and 50 into the walk.  Here the two halves are separate launches, built from the
// same routines as k_fx_nodes (fx_walk_node, fx_root_clusters, fx_test_children, fx_test_root, fx_run_job, fx_queue_layer2, ...);
// what is their own is the hand-over between them:
//   k_fx_walk<L>   the walk with two list chains in flight instead of four (no PCA: <= 256 VGPRs) and the root node's temporal
//                  clusters when some root spans several bins (root_multi; its bins are summed in LDS during the walk).  Per
//                  wavefront it leaves 11 words per child (n | clusters, St, Sq, Sqq; lane-contiguous), a 256-byte descriptor
//                  (the parents' blocks and keys, the roots' cluster counts) and its jobs in a pool; list heads are cleared
//                  behind it.
//   k_fx_test<L>   the same wavefront-to-parents mapping, read from the descriptor (one round of loads, nothing to search): node
//                  tests, emission, the jobs from the pool, the layer-2 queue, header + hash entry cleared behind it.
// The output of a sweep does not depend on which form ran (tests/test_extract_gpu.py compares the bytes).

constexpr int kFxNodeW = 11;      // u64 words per child node: n | ncl << 32, St, Sq[3], Sqq[6]
constexpr int kFxDescW = 64;      // u32 words per wavefront descriptor: 8 x {block index, key, flags, spare} | jobs | job base
constexpr int kFxWalkChains = 2;  // list chains in flight per lane (k_fx_merge leaves lists of one record)
constexpr uint32_t kFxJobSub0 = 8;  // job sub-pool counters: sub-counters 8..15 of the spill bank (the spill pool uses 0..7)
// (the codes of a job's PCA near a gate, 17 + FxPca::which, overlap the walk's own 17 ... 19)
constexpr FxWhy kFxWhySplit = {17, 23, 18, 19, 20, 21, 17};

template <int LEVEL>
__device__ __forceinline__ void fx_walk_body(const FxArgs &A, const uint32_t bid, const uint32_t nblk) {
  __shared__ uint32_t s_heads[64][kFxSlots + 1];
  __shared__ unsigned long long s_root[8][kFxSlots][13];
  const ExParams &P = A.P;
  const int lane = threadIdx.x, g = lane >> 3, gl = lane & 7;
  const uint32_t bank = LEVEL == 1 ? kFxStRoots : kFxStNodes2;
  const uint32_t per = LEVEL == 1 ? A.mr_per : A.mq_per;
  uint32_t total = 0, cnts[kFxSub];
#pragma unroll
  for (int j = 0; j < kFxSub; ++j) {
    cnts[j] = min(*fx_cnt(A, bank, j), per);
    total += cnts[j];
  }
  if (WC_DBG(P, 2048)) return;
  unsigned long long *jb = A.jobs + (size_t)bid * kFxJobCap * kFxJobW;  // staging area of this wavefront's jobs
  for (uint32_t it = 0;; ++it) {
    const uint32_t vw = bid + it * nblk;  // "virtual wavefront": eight consecutive parents of the dense lists
    const uint32_t w0 = vw * 8u;
    if (w0 >= total) break;
    const uint32_t gi = w0 + (uint32_t)g;
    const bool have_parent = gi < total;
    const uint32_t pidx = fx_dense_parent<LEVEL>(A, cnts, per, gi, have_parent);
    unsigned long long *blk = (LEVEL == 1 ? A.blk : A.blk2) + (size_t)pidx * kFxBlockW;
    uint32_t key, o1p, minbin;
    fx_parent_header<LEVEL>(A, blk, pidx, have_parent, key, o1p, minbin);
    const uint32_t occ = fx_load_heads(blk, have_parent, minbin, s_heads[lane]);
    uint32_t jcnt = 0;
    // the bins of the ROOT node (all children together): which ones exist is known from the children's masks
    uint32_t rocc = occ;
    if (LEVEL == 1) {
      for (int m = 1; m < 8; m <<= 1) rocc |= (uint32_t)__shfl_xor((int)rocc, m, 8);
    }
    const bool root_multi = LEVEL == 1 && __ballot(have_parent && (rocc & (rocc - 1u)) != 0u) != 0ull;  // some root spans several bins
    if (root_multi) {
      for (int i = lane; i < 8 * kFxSlots * 13; i += 64) (&s_root[0][0][0])[i] = 0ull;
      __builtin_amdgcn_wave_barrier();
    }
    auto push_job = [&](bool closing, const FxPart &cl, uint32_t ordv, uint32_t owner) {
      fx_push_job(A, jb, jcnt, closing, cl, ordv, owner, kFxWhySplit.jobs);
    };
    FxPart tot;
    uint32_t ncl;
    fx_walk_node<LEVEL, kFxWalkChains>(A, occ, minbin, s_heads[lane], root_multi, s_root[g], kFxWhySplit, push_job, tot, ncl);
    __builtin_amdgcn_wave_barrier();
    // ---- the root node's temporal clusters (LEVEL 1): only a root that holds more than min_points is ever tested, and only a
    //      root with several bins can have several clusters ----
    uint32_t root_ncl = 0;
    if (LEVEL == 1) {
      long long rn = (long long)tot.n;
      rn = fx_gsum8(rn);
      const bool rl = have_parent && gl == 0 && (int)rn > P.min_points;
      root_ncl = rl ? 1u : 0u;
      if (root_multi && __ballot(rl && (rocc & (rocc - 1u)) != 0u)) root_ncl = fx_root_clusters(A, rl, s_root[g], kFxWhySplit.gap, push_job);
    }
    // ---- what k_fx_test needs: the children's sums (word-major: every store is one 512-byte row), the descriptor, the jobs ----
    {
      unsigned long long *nd = A.nodes + (size_t)vw * kFxNodeW * 64 + lane;
      nd[0 * 64] = (unsigned long long)tot.n | ((unsigned long long)ncl << 32);
      nd[1 * 64] = (unsigned long long)tot.st;
#pragma unroll
      for (int i = 0; i < 3; ++i) nd[(2 + i) * 64] = (unsigned long long)tot.s[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) nd[(5 + i) * 64] = (unsigned long long)tot.ss[i];
      uint32_t *wd = A.wdesc + (size_t)vw * kFxDescW;
      if (gl == 0) {
        const uint32_t flags = (have_parent ? 1u : 0u) | (o1p << 1) | (min(root_ncl, 255u) << 8);
        *(uint4 *)(wd + 4 * g) = make_uint4(pidx, key, flags, 0u);
      }
      const uint32_t nj = min(jcnt, (uint32_t)kFxJobCap);
      uint32_t jbase = 0;
      if (nj) {  // the jobs move from the staging area to a pool k_fx_test reads them from (one atomic per wavefront with jobs)
        const uint32_t sp = vw & 7u;
        if (lane == 0) jbase = atomicAdd(fx_cnt(A, kFxStSpillBank, kFxJobSub0 + sp), nj);
        jbase = (uint32_t)__shfl((int)jbase, 0);
        if (jbase + nj > A.jobpool_per) {
          fx_fallback(A.status, 22);
        } else {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_wave_barrier();
          const unsigned long long *src = jb;
          unsigned long long *dst = A.jobpool + ((size_t)sp * A.jobpool_per + jbase) * kFxJobW;
          for (uint32_t i = (uint32_t)lane; i < nj * (uint32_t)kFxJobW; i += 64u)
            dst[i] = __hip_atomic_load(&src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (L2, where the stores went)
        }
      }
      if (lane == 0) *(uint2 *)(wd + 32) = make_uint2(nj, jbase);
    }
    if (have_parent && !(WC_DBG(P, 8192))) fx_clear_heads(blk);
    __builtin_amdgcn_wave_barrier();  // (the staging area and s_heads are reused by the next round)
  }
}

template <int LEVEL>
__device__ __forceinline__ void fx_test_body(const FxArgs &A, const uint32_t bid, const uint32_t nblk) {
  __shared__ uint8_t s_flag[72];  // owner (child lane | 64 + group) is a plane with several temporal clusters: its jobs are emitted
  __shared__ uint32_t s_gkey[8], s_go1p[8];
  const ExParams &P = A.P;
  const int lane = threadIdx.x, g = lane >> 3, gl = lane & 7;
  const uint32_t bank = LEVEL == 1 ? kFxStRoots : kFxStNodes2;
  const uint32_t per = LEVEL == 1 ? A.mr_per : A.mq_per;
  uint32_t total = 0;
#pragma unroll
  for (int j = 0; j < kFxSub; ++j) total += min(*fx_cnt(A, bank, j), per);
  double x0, y0, z0;
  ex_origin(A.pts, x0, y0, z0);
  const int k0x = vox(x0, P.vs), k0y = vox(y0, P.vs), k0z = vox(z0, P.vs);
  const float q0 = P.vs_f / 4;
  const uint32_t wsub = bid & (kFxSub - 1);
  if (WC_DBG(P, 2048)) return;
  for (uint32_t it = 0;; ++it) {
    const uint32_t vw = bid + it * nblk;
    if (vw * 8u >= total) break;
    // descriptor + sums of this wavefront's parents: one round of loads
    const uint32_t *wd = A.wdesc + (size_t)vw * kFxDescW;
    const uint4 d4 = *(const uint4 *)(wd + 4 * g);
    const uint2 dj = *(const uint2 *)(wd + 32);
    const unsigned long long *nd = A.nodes + (size_t)vw * kFxNodeW * 64 + lane;
    unsigned long long nw[kFxNodeW];
#pragma unroll
    for (int i = 0; i < kFxNodeW; ++i) nw[i] = nd[i * 64];
    const bool have_parent = (d4.z & 1u) != 0u;
    const uint32_t pidx = d4.x, key = d4.y, o1p = (d4.z >> 1) & 7u, root_ncl = (d4.z >> 8) & 0xFFu;
    const uint32_t jcnt = dj.x, jbase = dj.y;
    unsigned long long *blk = (LEVEL == 1 ? A.blk : A.blk2) + (size_t)pidx * kFxBlockW;
    int kx, ky, kz;
    double cc[3];
    fx_key_voxel(P, key, k0x, k0y, k0z, kx, ky, kz, cc);
    FxPart tot;
    fx_zero(tot);
    uint32_t ncl = 0;
    if (have_parent) {
      tot.n = (uint32_t)nw[0], ncl = (uint32_t)(nw[0] >> 32), tot.st = (long long)nw[1];
#pragma unroll
      for (int i = 0; i < 3; ++i) tot.s[i] = (long long)nw[2 + i];
#pragma unroll
      for (int i = 0; i < 6; ++i) tot.ss[i] = (long long)nw[5 + i];
    }
    FxPart rt;
    bool parent_live;
    uint32_t split;
    const FxEmit pend = fx_test_children<LEVEL>(A, have_parent, tot, ncl, key, o1p, kx, ky, kz, cc, q0, wsub, kFxWhySplit.slots, s_flag, s_gkey, s_go1p,
                                                rt, parent_live, split);
    if (LEVEL == 1) fx_test_root(A, parent_live, rt, cc, kx, ky, kz, q0, wsub, kFxWhySplit.slots, s_flag, [&](bool) { return root_ncl; });
    fx_emit_end(A, pend);
    __builtin_amdgcn_wave_barrier();
    // ---- the jobs, one lane each, from the pool k_fx_walk filled ----
    const unsigned long long *jp = A.jobpool + ((size_t)(vw & 7u) * A.jobpool_per + jbase) * kFxJobW;
    for (uint32_t r0 = 0; r0 < jcnt; r0 += 64u) {
      const uint32_t ji = r0 + (uint32_t)lane;
      bool want = ji < jcnt;
      unsigned long long w[kFxJobW];
#pragma unroll
      for (int i = 0; i < kFxJobW; ++i) w[i] = want ? jp[(size_t)ji * kFxJobW + i] : 0ull;
      const uint32_t owner = want ? min((uint32_t)w[11], 71u) : 0u;
      want = want && s_flag[owner] != 0;
      if (!__ballot(want)) continue;
      FxPart cl;
      fx_zero(cl);
      cl.n = (uint32_t)w[0], cl.st = (long long)w[1];
      const uint32_t ordv = (uint32_t)(w[0] >> 32);
#pragma unroll
      for (int i = 0; i < 3; ++i) cl.s[i] = (long long)w[2 + i];
#pragma unroll
      for (int i = 0; i < 6; ++i) cl.ss[i] = (long long)w[5 + i];
      fx_run_job<LEVEL>(A, want, owner, cl, ordv, k0x, k0y, k0z, q0, wsub, kFxWhySplit, s_gkey, s_go1p);
    }
    __builtin_amdgcn_wave_barrier();
    const bool queued = LEVEL == 1 && fx_queue_layer2(A, have_parent, split, pidx, key, blk, wsub);
    // (the list heads were cleared by k_fx_walk)
    if (have_parent && gl == 0 && !(WC_DBG(P, 8192))) fx_clear_header<LEVEL>(A, blk, pidx, queued);
    __builtin_amdgcn_wave_barrier();  // (s_flag / s_gkey are rewritten by the next round)
  }
}

template <int LEVEL>
__global__ void __launch_bounds__(64) k_fx_walk(FxArgs A) {
  fx_walk_body<LEVEL>(A, blockIdx.x, gridDim.x);
}
template <int LEVEL>
__global__ void __launch_bounds__(64) k_fx_test(FxArgs A) {
  fx_test_body<LEVEL>(A, blockIdx.x, gridDim.x);
}
template <int LEVEL>
__global__ void __launch_bounds__(64) k_fx_walk_b(FxBatch B) {
  uint32_t bid;
  const int k = fx_batch_find(B, blockIdx.x, bid);
  if (LEVEL == 2 && !(B.flags[k] & 1u)) return;
  WC_FX_BATCH_ARGS(sA, B, k)
  fx_walk_body<LEVEL>(sA, bid, B.start[k + 1] - B.start[k]);
}
template <int LEVEL>
__global__ void __launch_bounds__(64) k_fx_test_b(FxBatch B) {
  uint32_t bid;
  const int k = fx_batch_find(B, blockIdx.x, bid);
  if (LEVEL == 2 && !(B.flags[k] & 1u)) return;
  WC_FX_BATCH_ARGS(sA, B, k)
  fx_test_body<LEVEL>(sA, bid, B.start[k + 1] - B.start[k]);
}
