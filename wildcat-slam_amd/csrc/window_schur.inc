// window_schur.inc — the damped LM step with the bias unknowns eliminated first (included by window.hip behind the dense
// Cholesky kernels, whose panel steps, back substitution and lm_step it reuses).
//
// The reference asks Ceres for SPARSE_NORMAL_CHOLESKY (lidar_odometry.cc:553).  What is sparse in the window's normal
// equations: the six bias unknowns (bg, ba) of a sample state appear in IMU factors only (cost_functor.h:264-355), and an IMU
// factor touches three consecutive sample states (lidar_odometry.cc:319-363) - the bias x bias part of H is block
// pentadiagonal, the bias x pose part has five 6 x 6 blocks per block row; the pose x pose part is dense (surfel factors pair
// any two times of the window).  The dense factorisation of round 2 spends one ~9 us panel step per 32 unknowns, bias or not:
// 48 steps at 127 sample states.  Here the damped system  [T C; C^T P] [yB; yP] = [bB; bP]  (T: bias, P: pose) is solved as
//   X  = T^-1 [C | bB]          block tridiagonal in super-blocks of two sample states (12 x 12), ALL columns at once, by
//                               PARALLEL CYCLIC REDUCTION: ceil(log2(ns / 2)) levels, every block row active on every level -
//                               a sequential banded factorisation is a chain of 6 ns dependent pivots (~60 us at ns = 127,
//                               most of what the elimination saves); PCR is six launches of a few us
//   S  = P - C^T X,  c = bP - C^T x_b      30 multiply-adds per entry (C is banded), fused with the damping of P
//   S yP = c                    the dense blocked Cholesky of round 2 on HALF the unknowns (24 panel steps instead of 48)
//   yB = x_b - X yP             one matrix-vector product
// Same step as the dense path up to rounding (the elimination order differs); the oracle comparison of the solve holds both
// to 1e-6 (tests/test_window_gpu.py), the development option lm_dense keeps the dense path for A/B runs.

constexpr int kSB = 12;  // unknowns of a bias super-block: bg, ba of two consecutive sample states

// Workgroup p of a launch runs on XCD p % 8 (observed placement; MI355X_MICROARCH.md), and the eight XCDs' L2s do not share lines: a
// matrix every workgroup reads part of - X in k_schur_form (4.7 MB), R in a reduction level - is fetched once PER XCD that touches it.
// With neighbouring rows dealt round-robin over the XCDs every L2 pulls (nearly) all of it, ~8 x the bytes; this maps the launch's
// linear workgroup id to a logical id such that an XCD's workgroups are CONSECUTIVE logical ids (neighbouring rows -> the same L2).
// A bijection of [0, N) for any N; placement is an optimisation only, never correctness.
__device__ __forceinline__ uint32_t xcd_major(uint32_t p, uint32_t N) {
  const uint32_t c = p & 7u, slot = p >> 3, q = N >> 3, r = N & 7u;
  return c * q + (c < r ? c : r) + slot;
}

__device__ __forceinline__ int schur_orig_bias(int ib) { return 12 * (ib / 6) + 6 + ib % 6; }
__device__ __forceinline__ int schur_orig_pose(int ip) { return 12 * (ip / 6) + ip % 6; }

// level-0 blocks of the bias system, straight from the dense H: D(m) (12 x 12, damped), A(m) = coupling of super-block m to
// m - 1, R(m) = 12 rows of [C | bB | 0 ...].  A sample state beyond the window (odd ns) is an identity row.
struct PcrSrc {
  const double *H, *g, *scale;
  int n, ns;
  double radius;
  double *diag;
};
__device__ __forceinline__ void pcr_src_DA(const PcrSrc &P, int m, int e, double &d, double &a, bool write_diag) {
  const int r = e / kSB, c = e % kSB;
  const int ib = kSB * m + r, jb = kSB * m + c, kb = kSB * (m - 1) + c;
  const bool vr = ib / 6 < P.ns, vc = jb / 6 < P.ns;
  d = (r == c) ? 1.0 : 0.0, a = 0.0;
  if (vr && vc) {
    const int oi = schur_orig_bias(ib), oj = schur_orig_bias(jb);
    d = P.H[(size_t)oi * P.n + oj] * P.scale[oi] * P.scale[oj];
    if (r == c && P.radius > 0.0) {  // (radius 0: UNDAMPED - the first level adds the damping, pcr_damp)
      const double dd = fmin(fmax(d, 1e-6), 1e32);  // LM min / max diagonal, as damped_entry
      if (write_diag) P.diag[oi] = dd / P.radius;
      d += dd / P.radius;
    }
  } else if (vr != vc) {
    d = 0.0;
  }
  if (vr && m > 0) {
    const int oi = schur_orig_bias(ib), ok = schur_orig_bias(kb);
    a = P.H[(size_t)oi * P.n + ok] * P.scale[oi] * P.scale[ok];
  }
}
__device__ __forceinline__ double pcr_src_R(const PcrSrc &P, int m, int r, int col) {
  const int npz = 6 * P.ns;
  const int ib = kSB * m + r;
  if (ib / 6 >= P.ns || col > npz) return 0.0;
  const int ob = schur_orig_bias(ib);
  if (col == npz) return P.g[ob] * P.scale[ob];
  const int op = schur_orig_pose(col);
  return P.H[(size_t)ob * P.n + op] * P.scale[ob] * P.scale[op];
}

// (Round 3 also tried the whole reduction in TWO launches - one workgroup running all levels of the blocks, then one workgroup per eight
// right-hand-side columns keeping them in LDS through all levels: correct, and 792 + 67 us against 86: a single CU's load rate, not the
// launches, bounds it - every level re-reads its alpha / gamma / A blocks, 1 MB per level through one CU.  A launch per level stays.)
// level 0 as a pass of its own (fusing it into the first level - every block formed from H where it is used - measured 25.5 us
// against 9 + 12: the first level's loads then sit behind H's address arithmetic and branches)
__global__ void __launch_bounds__(256) k_pcr_init(PcrSrc P, double *D, double *A, double *R, int ldr, int *fail) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const int col = blockIdx.y * 256 + tid;
  if (col < ldr) {
#pragma unroll
    for (int r = 0; r < kSB; ++r) R[(size_t)(kSB * m + r) * ldr + col] = pcr_src_R(P, m, r, col);
  }
  if (blockIdx.y == 0) {
    if (m == 0 && tid == 0) *fail = 0;
    for (int e = tid; e < kSB * kSB; e += 256) {
      double d, a;
      pcr_src_DA(P, m, e, d, a, true);
      D[(size_t)m * 144 + e] = d;
      A[(size_t)m * 144 + e] = a;
    }
  }
}

// In-place inverses of `count` (1 or 2) symmetric positive definite 12 x 12 matrices in LDS (Gauss-Jordan without pivoting: the blocks
// are Schur complements of a damped SPD matrix), ONE WAVEFRONT per matrix, the matrix in REGISTERS: lane c < 12 holds column c; a pivot step takes the pivot
// and column k from lane k with v_readlane (the loop is unrolled: register indices and lane numbers are constants), row k is the
// lane's own register k.  No LDS traffic and no barrier inside the twelve steps.  Entry by entry the arithmetic of the workgroup-wide
// Gauss-Jordan of round 3 (256 threads, two barriers per pivot step): the same bits - checked on the solve's x,
// profiles/dev/lm_repeat.py.  A knock-out build (profiles/dev/pcr_knock.sh) had put the two inverses of a level at 3.6 of its 10.5 us;
// one wavefront per matrix with the matrix in LDS (in-order LDS operations instead of barriers) made them 2.3, this form ~1.
// A non-positive pivot is reported to *fail by the wavefront that meets it.  The caller synchronises the workgroup behind the call.
__device__ __forceinline__ void gj_inv12_wave(double (*S)[kSB][kSB + 2], int count, int *fail) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (w >= count) return;
  double (*M)[kSB + 2] = S[w];
  const int c = lane < kSB ? lane : 0;
  double a[kSB];
#pragma unroll
  for (int r = 0; r < kSB; ++r) a[r] = M[r][c];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < kSB; ++k) {
    const double p = readlane_d(a[k], k);
    if (!(p > 0.0)) ok = false;
    double ip = __builtin_amdgcn_rcp(p);  // (estimate + two Newton steps: <= 2 ulp, a third of the IEEE division's chain)
    ip = fma(fma(-p, ip, 1.0), ip, ip);
    ip = fma(fma(-p, ip, 1.0), ip, ip);
    const double skj = a[k];
    double nv[kSB];
#pragma unroll
    for (int r = 0; r < kSB; ++r) {
      const double sik = readlane_d(a[r], k), old = a[r];
      nv[r] = (r == k) ? (c == k ? ip : skj * ip) : (c == k ? -sik * ip : fma(-sik * ip, skj, old));
    }
#pragma unroll
    for (int r = 0; r < kSB; ++r) a[r] = nv[r];
  }
  if (lane < kSB) {
#pragma unroll
    for (int r = 0; r < kSB; ++r) M[r][c] = a[r];
  }
  if (!ok && lane == 0) atomicOr(fail, 1);
}

// (Round 3, second half, tried instead of the levels: a TWISTED block elimination - one wavefront per (direction, 64 right-hand-
// side columns) walks from its end of the chain to the middle, E(m) = D(m) - A(m) E(m-1)^-1 A(m)^T on 12 x 12 blocks in LDS with a
// barrier-free in-wavefront Gauss-Jordan inverse, a second launch solves the two middle rows and substitutes back: two launches
// of M / 2 dependent steps.  Correct (all solve tests), and 172 us against 64 for the 32 super-blocks of the odometry step's
// window: a step is ~5 us of LDS round trips and reciprocal chains in ONE wavefront, not the 1 us it would have to be.  The
// levels stay.)
// (Round 4, tried: TWO levels per launch - the workgroup of row m forms the stride-s rows m - 2 s, m, m + 2 s itself from the seven rows
// m - 3 s ... m + 3 s and absorbs the outer two, every sum in this kernel's order: the same bits (checksum of the solve's x), one launch
// less per pair of levels - and 24 us MORE per LM iteration of the odometry step (solve 2.13 -> 2.32 ms): 84 right-hand-side values and
// 290 registers per thread, one wavefront per SIMD, three times the sums per workgroup; a level's ~10 us are not its launch.)
// one level of parallel cyclic reduction at stride s: row m absorbs rows m - s and m + s,
//   alpha = -A[m] D[m-s]^-1, gamma = -A[m+s]^T D[m+s]^-1
//   D'[m] = D[m] + alpha A[m]^T + gamma A[m+s];  A'[m] (to m - 2 s) = alpha A[m-s];  R'[m] = R[m] + alpha R[m-s] + gamma R[m+s]
// grid = (M, column chunks of 256): every workgroup forms alpha / gamma itself (two 12 x 12 inverses), chunk 0 writes D', A'.
// LAST: the rows leave this level decoupled, so the workgroup inverts its own D'[m] and writes X[m] = D'[m]^-1 R'[m] instead of
// R' (no launch of its own for that).
// Round 5: the level-0 blocks leave k_pcr_init UNDAMPED and the first level adds the LM damping where it reads a D block - entry
// (r, r) of super-block mm, a real sample state's bias unknown: d + clamp(d) / radius, the expression of pcr_src_DA.  k_pcr_init then
// does not depend on the trust-region radius and is enqueued right behind the candidate's linearisation, before the host has the
// mailbox of the iteration: when the step is accepted - the rule - the next iteration starts with its first level (the 7 - 12 us of
// k_pcr_init ran in the 10 - 14 us the device idled between two iterations).
struct PcrDamp {
  double radius;  // 0: the blocks are damped already
  int ns;
  double *diag;
};
__device__ __forceinline__ double pcr_damp(const PcrDamp &Q, int mm, int e, double d) {
  const int r = e / kSB, c = e % kSB;
  if (r != c || (kSB * mm + r) / 6 >= Q.ns) return d;
  return d + fmin(fmax(d, 1e-6), 1e32) / Q.radius;
}
template <bool LAST, bool FIRST>
__global__ void __launch_bounds__(256) k_pcr_level(int s, int M, const double *__restrict__ Din, const double *__restrict__ Ain,
                                                  const double *__restrict__ Rin, double *Dout, double *Aout, double *Rout, int ldr, int *fail,
                                                  PcrDamp Q, int npz, int limited) {
  __shared__ __align__(16) double sI[2][kSB][kSB + 2];  // (rows of 14 doubles: the last level reads its inverse two entries at a time)
  __shared__ double sAl[kSB][kSB + 1], sAu[kSB][kSB + 1], sALL[kSB][kSB + 1], sDm[kSB][kSB + 1];
  // (alpha / gamma in rows of 14 doubles, 16-byte aligned: the right-hand sides' update reads them two at a time - 144 LDS reads per
  // thread instead of 288; they were 2.7 of a level's 10.5 us in the knock-out build)
  __shared__ __align__(16) double sAlpha[kSB][kSB + 2], sGamma[kSB][kSB + 2];
  // (a 1-D launch of M x column chunks workgroups, XCD-major: the rows m - s, m, m + s a workgroup reads are - for the small strides -
  // rows its XCD's other workgroups read as well)
  const uint32_t lg_ = xcd_major(blockIdx.x, gridDim.x);
  const int m = (int)(lg_ % (uint32_t)M), chunk_ = (int)(lg_ / (uint32_t)M), tid = threadIdx.x;
  const int L = m - s, U = m + s;
  const bool hasL = L >= 0, hasU = U < M;
  auto ldR = [&](int mm, int r, int col) -> double { return Rin[(size_t)(kSB * mm + r) * ldr + col]; };
  // this thread's column of the three rows' right-hand sides: requested before the inverses (their latency runs beside them)
  // Round 6: the right-hand sides are BANDED while the strides are small.  Row mm of [C | b] starts with the pose columns of super-blocks
  // mm - 1 .. mm + 1 (an IMU factor couples three consecutive sample states) plus the b column; a level of stride s reads rows whose band
  // is s super-blocks wide to either side and leaves one 2 s wide.  `limited`: the workgroups of row m cover only the columns of ITS
  // output band (12 (4 s + 1): one chunk of 256 up to s = 4, two at s = 8, instead of ldr / 256 everywhere), the last thread of the last
  // chunk takes the b column; nobody writes outside a band, so what lies there is stale and every load is masked by its SOURCE row's band
  // (in every level: the full-width ones read the banded ones' output).
  int col = chunk_ * 256 + tid;
  bool live = col < ldr;
  if (limited) {
    const int c0 = kSB * max(0, m - 2 * s), c1 = min(npz, kSB * (m + 2 * s + 1));
    col = c0 + chunk_ * 256 + tid;
    live = col < c1;
    if (chunk_ == limited - 1 && tid == 255) col = npz, live = true;  // (its own column lies beyond the band: 256 x chunks > 12 (4 s + 1))
  }
  auto in_band = [&](int mm) -> bool { return col == npz || (col >= kSB * (mm - s) && col < kSB * (mm + s + 1)); };
  double rl[kSB], ru[kSB], rm[kSB];
  const bool okL = live && hasL && in_band(L), okU = live && hasU && in_band(U), okM = live && in_band(m);
#pragma unroll
  for (int k = 0; k < kSB; ++k) {
    rl[k] = okL ? ldR(L, k, col) : 0.0;
    ru[k] = okU ? ldR(U, k, col) : 0.0;
    rm[k] = okM ? ldR(m, k, col) : 0.0;
  }
  // every block this row needs, one entry per thread and block, all requests in one round
  const bool needDA = LAST || chunk_ == 0;  // D[m] and A[m - s]: for D'[m] / A'[m]
  for (int e = tid; e < 144; e += 256) {
    const int r = e / kSB, c = e % kSB;
    double dL = (r == c ? 1.0 : 0.0), dU = dL, dM = 0.0, aM = 0.0, aU = 0.0, aL = 0.0;
    if (hasL) dL = Din[(size_t)L * 144 + e], aM = Ain[(size_t)m * 144 + e], aL = Ain[(size_t)L * 144 + e];
    if (hasU) dU = Din[(size_t)U * 144 + e], aU = Ain[(size_t)U * 144 + e];
    if (needDA) dM = Din[(size_t)m * 144 + e];
    if (FIRST) {
      if (hasL) dL = pcr_damp(Q, L, e, dL);
      if (hasU) dU = pcr_damp(Q, U, e, dU);
      if (needDA) {
        const double dm0 = dM;
        dM = pcr_damp(Q, m, e, dM);
        if (chunk_ == 0 && r == c && (kSB * m + r) / 6 < Q.ns) Q.diag[schur_orig_bias(kSB * m + r)] = fmin(fmax(dm0, 1e-6), 1e32) / Q.radius;  // (what lm_step's model reads)
      }
    }
    sI[0][r][c] = dL, sI[1][r][c] = dU, sAl[r][c] = aM, sAu[r][c] = aU, sALL[r][c] = (L - s >= 0) ? aL : 0.0, sDm[r][c] = dM;
  }
  __syncthreads();
  gj_inv12_wave(sI, 2, fail);
  __syncthreads();
  for (int e = tid; e < 288; e += 256) {
    const int which = e / 144, r = (e % 144) / kSB, c = e % kSB;
    double acc = 0.0;
    if (which == 0) {
#pragma unroll
      for (int k = 0; k < kSB; ++k) acc = fma(sAl[r][k], sI[0][k][c], acc);
      sAlpha[r][c] = -acc;
    } else {
#pragma unroll
      for (int k = 0; k < kSB; ++k) acc = fma(sAu[k][r], sI[1][k][c], acc);
      sGamma[r][c] = -acc;
    }
  }
  __syncthreads();
  // D'[m] (every workgroup of a LAST level needs it; otherwise chunk 0 alone) and A'[m]
  if (LAST || chunk_ == 0) {
    const bool hasLL = L - s >= 0;
    for (int e = tid; e < 144; e += 256) {
      const int r = e / kSB, c = e % kSB;
      double d = sDm[r][c], a = 0.0;
#pragma unroll
      for (int k = 0; k < kSB; ++k) d = fma(sAlpha[r][k], sAl[c][k], fma(sGamma[r][k], sAu[k][c], d));
      if (hasLL && !LAST) {
#pragma unroll
        for (int k = 0; k < kSB; ++k) a = fma(sAlpha[r][k], sALL[k][c], a);
      }
      if (LAST) {
        sI[0][r][c] = d;
      } else {
        Dout[(size_t)m * 144 + e] = d;
        Aout[(size_t)m * 144 + e] = a;
      }
    }
  }
  double rn[kSB];
#pragma unroll
  for (int r = 0; r < kSB; ++r) {
    double v = rm[r];
#pragma unroll
    for (int k = 0; k < kSB; k += 2) {  // (the same sums in the same order)
      const double2 al = *(const double2 *)&sAlpha[r][k], ga = *(const double2 *)&sGamma[r][k];
      v = fma(al.x, rl[k], fma(ga.x, ru[k], v));
      v = fma(al.y, rl[k + 1], fma(ga.y, ru[k + 1], v));
    }
    rn[r] = v;
  }
  if (LAST) {
    __syncthreads();
    gj_inv12_wave(sI, 1, fail);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSB; ++r) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < kSB; k += 2) {  // (the same sum in the same order)
        const double2 iv = *(const double2 *)&sI[0][r][k];
        v = fma(iv.x, rn[k], v);
        v = fma(iv.y, rn[k + 1], v);
      }
      if (live) Rout[(size_t)(kSB * m + r) * ldr + col] = v;  // X[m]
    }
  } else if (live) {
#pragma unroll
    for (int r = 0; r < kSB; ++r) Rout[(size_t)(kSB * m + r) * ldr + col] = rn[r];
  }
}

// entry (i, j), j <= i, of the reduced, damped, augmented system (np2 x np2, the layout k_chol_step works on): the Schur
// complement S = P - C^T X for pose unknowns, row npz = (bP - C^T x_b)^T, padding = identity.  C's entries come straight from H
// (bias rows of the five sample states around the pose unknown's own).
__device__ __forceinline__ double schur_entry(const double *__restrict__ H, const double *__restrict__ g, const double *__restrict__ scale,
                                              const double *__restrict__ X, int n, int ns, int ldr, double radius, int i, int j, double *diag_out) {
  const int npz = 6 * ns;
  if (i > npz) return i == j ? 1.0 : 0.0;
  if (i == npz && j == npz) return 1e300;  // the corner only has to keep the pivot positive (as in damped_entry)
  // pose unknown whose coupling column is walked: column i of C for a matrix row, column j for the augmented row
  const int pc = i < npz ? i : j;
  const int opc = schur_orig_pose(pc);
  const int xcol = i < npz ? j : npz;  // X column: the pose unknown j, or x_b
  double v;
  if (i < npz) {
    const int oi = opc, oj = schur_orig_pose(j);
    v = H[(size_t)oi * n + oj] * scale[oi] * scale[oj];
    if (i == j) {
      const double d = fmin(fmax(v, 1e-6), 1e32);
      if (diag_out) diag_out[oi] = d / radius;
      v += d / radius;
    }
  } else {
    v = g[opc] * scale[opc];
  }
  const int sp = pc / 6;
  const int s0 = max(0, sp - 2), s1 = min(ns - 1, sp + 2);
  const double spc = scale[opc];
  (void)s0, (void)s1;
  // all 30 couplings requested before the first is used (a loop of dependent load - multiply - add steps is 30 round trips:
  // the lead workgroup of k_schur_form, which forms its 32 x 32 corner this way, lasted 15 us)
  double hv[30], sv[30], xv[30];
#pragma unroll
  for (int t = 0; t < 30; ++t) {
    const int sb = sp - 2 + t / 6, c = t % 6;
    const bool in = sb >= 0 && sb < ns;
    const int ob = in ? 12 * sb + 6 + c : 0, ib = in ? 6 * sb + c : 0;
    hv[t] = in ? H[(size_t)ob * n + opc] : 0.0;
    sv[t] = in ? scale[ob] : 0.0;
    xv[t] = in ? X[(size_t)ib * ldr + xcol] : 0.0;
  }
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < 30; ++t) acc = fma(hv[t] * sv[t] * spc, xv[t], acc);
  return v - acc;
}

// the reduced system into A (rows 1.. of the grid) and, workgroup (0, 0), the factor + inverse of its first diagonal block
// (the k_damp_first of the dense path)
__global__ void __launch_bounds__(256) k_schur_form(const double *__restrict__ H, const double *__restrict__ g, const double *__restrict__ scale,
                                                   const double *__restrict__ X, int n, int ns, int ldr, int np2, int ld2, double radius, double *A,
                                                   double *diag, double *Lmat, double *Linv, int *fail, int gx) {
  // (1-D launch, XCD-major: the six rows of a sample state read the 30 rows of X around it - 24 of them are the next sample state's too)
  const uint32_t lg_ = xcd_major(blockIdx.x, gridDim.x);
  const int bx_ = (int)(lg_ % (uint32_t)gx), by_ = (int)(lg_ / (uint32_t)gx);
  if (by_ == 0) {
    if (bx_ != 0) return;
    __shared__ double sB[kNB][kNB + 1];
    __shared__ double sXi[kNB][kNB + 1];
    // its 32 x 32 corner: pose unknowns of the first six sample states, whose couplings reach the bias rows of the first eight
    // (48 rows).  C[.][i] and X[.][j] of those rows are staged in LDS in ONE round of loads (the entries formed one by one, 30
    // couplings each, were a chain of ~15 us in front of the 5 us factor); couplings outside a row's band are exact zeros of H.
    constexpr int kLB = 48;
    __shared__ double sCc[kLB][kNB + 1], sXs[kLB][kNB + 1];
    const int nbr = min(kLB, 6 * ns), npz0 = 6 * ns;
    for (int e = threadIdx.x; e < kLB * kNB; e += 256) {
      const int ib = e / kNB, c = e % kNB;
      const bool in = ib < nbr && c < npz0;
      const int ob = in ? schur_orig_bias(ib) : 0, op = in ? schur_orig_pose(c) : 0;
      sCc[ib][c] = in ? H[(size_t)ob * n + op] * scale[ob] * scale[op] : 0.0;
      sXs[ib][c] = in ? X[(size_t)ib * ldr + c] : 0.0;
    }
    double own[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // the pose x pose part of this thread's four entries, in the same round
      const int e = threadIdx.x + 256 * q, r = e / kNB, c = e % kNB;
      double v = 0.0;
      if (c <= r && r < npz0) {
        const int oi = schur_orig_pose(r), oj = schur_orig_pose(c);
        v = H[(size_t)oi * n + oj] * scale[oi] * scale[oj];
        if (r == c) v += fmin(fmax(v, 1e-6), 1e32) / radius;
      }
      own[q] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = threadIdx.x + 256 * q, r = e / kNB, c = e % kNB;
      double v = 0.0;
      if (c <= r) {
        if (r < npz0) {
          double acc = 0.0;
          for (int ib = 0; ib < kLB; ++ib) acc = fma(sCc[ib][r], sXs[ib][c], acc);
          v = own[q] - acc;
        } else {
          v = schur_entry(H, g, scale, X, n, ns, ldr, radius, r, c, nullptr);  // (windows of fewer than six sample states)
        }
      }
      sB[r][c] = v;
    }
    __syncthreads();
    const bool ok = factor_inv32_roles(sB, sXi);
    if (threadIdx.x == 0 && !ok) atomicOr(fail, 1);
    __syncthreads();
    for (int e = threadIdx.x; e < kNB * kNB; e += 256) {
      const int r = e / kNB, c = e % kNB;
      Lmat[(size_t)r * ld2 + c] = sB[r][c];
      Linv[e] = sXi[r][c];
    }
    return;
  }
  // grid rows 1 .. ns: the six rows of one sample state's pose unknowns.  They share the 30 rows of X their couplings meet (bias
  // rows of the five sample states around it): a thread (= column j) fetches those 30 values ONCE and forms its entry of all
  // six rows - one row per workgroup read 138 MB of X per LM iteration out of L2 (22 us); the 30 coupling entries C[.][i] of
  // each row are staged in LDS
  __shared__ double sC[6][30];
  const int npz = 6 * ns;
  const int j = bx_ * blockDim.x + threadIdx.x;
  if (by_ > ns) {  // the augmented row (its couplings change with the column) and the padding: the general expression
    const int i = npz + by_ - ns - 1;
    if (i < np2 && j < np2 && j <= i) A[(size_t)i * ld2 + j] = schur_entry(H, g, scale, X, n, ns, ldr, radius, i, j, diag);
    return;
  }
  const int sp = by_ - 1;
  if (threadIdx.x < 180) {
    const int r = (int)threadIdx.x / 30, t = (int)threadIdx.x % 30;
    const int sb = sp - 2 + t / 6, c = t % 6;
    const bool in = sb >= 0 && sb < ns;
    const int opc = 12 * sp + r, ob = in ? 12 * sb + 6 + c : 0;
    sC[r][t] = in ? H[(size_t)ob * n + opc] * scale[ob] * scale[opc] : 0.0;
  }
  __syncthreads();
  if (j >= np2 || j > 6 * sp + 5) return;
  double xv[30];
#pragma unroll
  for (int t = 0; t < 30; ++t) {
    const int sb = sp - 2 + t / 6;
    xv[t] = (sb >= 0 && sb < ns) ? X[(size_t)(6 * sb + t % 6) * ldr + j] : 0.0;
  }
  const int oj = j < npz ? schur_orig_pose(j) : 0;
  const double sj = scale[oj];
  // (the six rows' entries of H and their scales in ONE round of loads: inside the loop below every load waited behind the stores of the
  // row before it - A and diag may alias H for all the compiler knows -, six dependent round trips per workgroup; round 6)
  double hv6[6], sc6[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    hv6[r] = H[(size_t)(12 * sp + r) * n + oj];
    sc6[r] = scale[12 * sp + r];
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int i = 6 * sp + r;
    if (j > i) continue;
    const int oi = 12 * sp + r;
    double v = hv6[r] * sc6[r] * sj;
    if (i == j) {
      const double d = fmin(fmax(v, 1e-6), 1e32);
      diag[oi] = d / radius;
      v += d / radius;
    }
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 30; ++t) acc = fma(sC[r][t], xv[t], acc);  // (same order as schur_entry: ascending bias row)
    A[(size_t)i * ld2 + j] = v - acc;
  }
}

// yB = x_b - X yP, both halves of y back in the order of the unknowns, four bias rows per workgroup (64 lanes each), and lm_step.
// Round 6: one launch instead of rounds 2 - 5's two, without a second look at y.  A workgroup forms its four bias rows of y (workgroup
// 0 also moves the pose half), and right there their part of lm_step: candidate entries xc / host_xc and the partial sums of the model
// cost change, |step|^2, |x|^2 and max |g| over the entries it owns.  The partials go to `part` (four doubles per workgroup) as
// agent-scope atomic stores, acknowledged (vmcnt) before the workgroup is counted; the workgroup that counts last adds the partials in
// workgroup order (fixed) and writes the mailbox's scalars.  No fence, no L2 write-back: the first form of this kernel - release fence
// per workgroup, acquire + lm_step over all of y in the last - took 15.6 us at 127 sample states against 12.2 for the two launches.
// (The scalars differ from the two launches' in the last bits - another summation order; they feed tolerances of 1e-3 and more.)
__global__ void __launch_bounds__(256) k_schur_bias_y_step(const double *__restrict__ X, const double *__restrict__ yred, int ns, int ldr, double *y,
                                                           StepArgs S, int n, uint32_t *done, double *part) {
  __shared__ uint32_t s_last;
  __shared__ double sp[4][4];
  const int npz = 6 * ns;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int ib = blockIdx.x * 4 + w;
  double mc = 0.0, sn = 0.0, xn = 0.0, gm = 0.0;
  auto entry = [&](int i, double yi, double sc, double gi, double xi, double di) {  // unknown i of the full system: lm_step's body
    const double d = -yi * sc;
    y[i] = yi;
    S.xc[i] = xi + d;
    S.host_xc[i] = xi + d;
    mc += yi * (gi * sc) + di * yi * yi;
    sn += d * d;
    xn += xi * xi;
    gm = fmax(gm, fabs(gi));
  };
  // this wavefront's bias unknown: its scale / g / x / diag are requested before the row's product (their latency runs beside it)
  const int ob = ib < npz ? schur_orig_bias(ib) : 0;
  const double b_sc = S.scale[ob], b_g = S.g[ob], b_x = S.x[ob], b_d = S.diag[ob];
  if (blockIdx.x == 0)  // (and the pose half)
    for (int q = tid; q < npz; q += 256) {
      const int i = schur_orig_pose(q);
      entry(i, yred[q], S.scale[i], S.g[i], S.x[i], S.diag[i]);
    }
  if (ib < npz) {
    const double *row = X + (size_t)ib * ldr;
    double acc = 0.0;
    int q = lane;
    for (; q + 192 < npz; q += 256) {  // (four independent loads per round; the same sums in the same order)
      const double r0 = row[q], r1 = row[q + 64], r2 = row[q + 128], r3 = row[q + 192];
      const double y0 = yred[q], y1 = yred[q + 64], y2 = yred[q + 128], y3 = yred[q + 192];
      acc = fma(r3, y3, fma(r2, y2, fma(r1, y1, fma(r0, y0, acc))));
    }
    for (; q < npz; q += 64) acc = fma(row[q], yred[q], acc);
    for (int mm = 32; mm >= 1; mm >>= 1) acc += __shfl_xor(acc, mm);
    if (lane == 0) entry(ob, row[npz] - acc, b_sc, b_g, b_x, b_d);
  }
  // the wavefront's sums by shuffles (fixed tree), the four wavefronts' in order
  for (int mm = 32; mm >= 1; mm >>= 1) {
    mc += __shfl_xor(mc, mm), sn += __shfl_xor(sn, mm), xn += __shfl_xor(xn, mm);
    gm = fmax(gm, __shfl_xor(gm, mm));
  }
  if (lane == 0) sp[0][w] = mc, sp[1][w] = sn, sp[2][w] = xn, sp[3][w] = gm;
  __syncthreads();
  if (tid == 0) {
    const double p0 = (sp[0][0] + sp[0][1]) + (sp[0][2] + sp[0][3]), p1 = (sp[1][0] + sp[1][1]) + (sp[1][2] + sp[1][3]);
    const double p2 = (sp[2][0] + sp[2][1]) + (sp[2][2] + sp[2][3]), p3 = fmax(fmax(sp[3][0], sp[3][1]), fmax(sp[3][2], sp[3][3]));
    __hip_atomic_store(&part[4 * blockIdx.x + 0], p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&part[4 * blockIdx.x + 1], p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&part[4 * blockIdx.x + 2], p2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&part[4 * blockIdx.x + 3], p3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t prev = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  mc = sn = xn = gm = 0.0;
  for (int b0 = 0; b0 < (int)gridDim.x; b0 += 256) {  // (fixed assignment and order: the same bits in every run)
    const int b = b0 + tid;
    if (b < (int)gridDim.x) {
      const double a0 = __hip_atomic_load(&part[4 * b + 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double a1 = __hip_atomic_load(&part[4 * b + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double a2 = __hip_atomic_load(&part[4 * b + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double a3 = __hip_atomic_load(&part[4 * b + 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      mc += a0, sn += a1, xn += a2, gm = fmax(gm, a3);
    }
  }
  for (int mm = 32; mm >= 1; mm >>= 1) {
    mc += __shfl_xor(mc, mm), sn += __shfl_xor(sn, mm), xn += __shfl_xor(xn, mm);
    gm = fmax(gm, __shfl_xor(gm, mm));
  }
  __syncthreads();
  if (lane == 0) sp[0][w] = mc, sp[1][w] = sn, sp[2][w] = xn, sp[3][w] = gm;
  __syncthreads();
  if (tid == 0) {
    S.mail[kMailModelChange] = 0.5 * ((sp[0][0] + sp[0][1]) + (sp[0][2] + sp[0][3]));
    S.mail[kMailStepNorm] = sqrt((sp[1][0] + sp[1][1]) + (sp[1][2] + sp[1][3]));
    S.mail[kMailXNorm] = sqrt((sp[2][0] + sp[2][1]) + (sp[2][2] + sp[2][3]));
    S.mail[kMailCost] = S.lin_cost[0];
    S.mail[kMailGmax] = fmax(fmax(sp[3][0], sp[3][1]), fmax(sp[3][2], sp[3][3]));
    __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
