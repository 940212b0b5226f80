// fx_eig3.h — the closed-form symmetric 3x3 eigen-solver of the default extraction path and its two hardware-estimate helpers, shared by
// extract_fast.inc (every surfel of a sweep) and map.hip (the plane of a map voxel).  Included inside the including file's anonymous
// namespace, after dmath.h; compile with -ffp-contract=off like every translation unit here.
#ifndef WC_FX_EIG3_H_
#define WC_FX_EIG3_H_
// Eigen-decomposition of a symmetric 3x3 matrix in closed form (trigonometric solution of the characteristic cubic): a tenth
// of the cyclic Jacobi iteration's cost.  The smallest eigenvalue - the one every gate and every surfel uses - is well
// conditioned here exactly when the matrix is plane-like; the result is only accepted when its residual is at rounding
// level, otherwise the Jacobi iteration of the exact path decides.
// 1 / x and 1 / sqrt(x) from the hardware estimates (v_rcp_f64 / v_rsq_f64, ~2^-26) and Newton steps: <= 2 ulp, a quarter of
// the clocks of the IEEE division / square root sequences - and fx_pca is 40 % of a k_fx_nodes wavefront (a dependent chain)
__device__ __forceinline__ double fx_rcp(double a) {
  double r = __builtin_amdgcn_rcp(a);
  r = fma(fma(-a, r, 1.0), r, r);
  return fma(fma(-a, r, 1.0), r, r);
}
__device__ __forceinline__ double fx_rsqrt(double a) {
  double r = __builtin_amdgcn_rsq(a);
  r = fma(0.5 * r, fma(-a * r, r, 1.0), r);
  return fma(0.5 * r, fma(-a * r, r, 1.0), r);
}
// accepted (the self-test's view, wc_selftest_fx_eig3): whether the closed form's result was taken or the Jacobi iteration decided
__device__ __forceinline__ void fx_eig3(const wc::M3 &A, double ev[3], wc::M3 &V, bool *accepted = nullptr) {
  const double a00 = A.m[0][0], a11 = A.m[1][1], a22 = A.m[2][2], a01 = A.m[0][1], a02 = A.m[0][2], a12 = A.m[1][2];
  const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
  const double q = (a00 + a11 + a22) * (1.0 / 3.0);
  const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
  const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * p1;
  bool ok = p2 > 0.0 && p1 > 0.0;
  if (ok) {
    const double p26 = p2 * (1.0 / 6.0), ip = fx_rsqrt(p26), p = p26 * ip;
    const double c00 = b00 * ip, c11 = b11 * ip, c22 = b22 * ip, c01 = a01 * ip, c02 = a02 * ip, c12 = a12 * ip;
    double r = 0.5 * (c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) + c02 * (c01 * c12 - c11 * c02));
    r = min(1.0, max(-1.0, r));
    // The eigenvalues are q + 2 p cos(theta_k), theta_k = (acos(r) + 2 pi k) / 3: the three roots of 4 x^3 - 3 x = r.  For
    // r <= 0 the SMALLEST root t in [-1, -sqrt(3)/2] is simple and well separated (r = -1: two equal large eigenvalues, the
    // isotropic plane patch), for r >= 0 the LARGEST root c in [sqrt(3)/2, 1] is (r = 1: two equal small eigenvalues, a line);
    // Newton from the outer end of the interval (f' >= 6 there, f monotone and of one curvature: no overshoot), starting on the
    // tangent at +-1, reaches it in five steps; the other extreme root follows from cos(theta -+ 2 pi / 3).  acos + sincos cost
    // eight times as much, and this routine is 40 % of a k_fx_nodes wavefront.  The residual test below still decides.
    const double sg = r <= 0.0 ? -1.0 : 1.0, ra = fabs(r);  // by symmetry solve 4 x^3 - 3 x = |r| for its largest root x
    double x = 1.0 - (1.0 - ra) * (1.0 / 9.0);
#pragma unroll
    for (int it = 0; it < 5; ++it) {
      const double x2 = x * x;
      x -= ((4.0 * x2 - 3.0) * x - ra) * __builtin_amdgcn_rcp(12.0 * x2 - 3.0);  // (the estimate will do: Newton corrects itself)
    }
    x = fmin(x, 1.0);
    // with x = cos(phi): -cos(phi + 2 pi / 3) = x / 2 + sqrt(3) / 2 sin(phi) =: z.  r >= 0: largest root x, smallest -z;
    // r < 0: the roots are the negated roots of |r|: smallest -x, largest z
    const double z = 0.5 * x + 0.8660254037844386 * sqrt(fmax(1.0 - x * x, 0.0));
    const double t = sg < 0.0 ? -x : -z;
    const double e0 = q + 2.0 * p * t;     // smallest
    // eigenvector of the smallest eigenvalue: the largest of the cross products of the rows of A - e0 I
    const double m00 = a00 - e0, m11 = a11 - e0, m22 = a22 - e0;
    const double x0 = a01 * a12 - a02 * m11, y0 = a02 * a01 - m00 * a12, z0 = m00 * m11 - a01 * a01;  // row0 x row1
    const double x1 = a01 * m22 - a02 * a12, y1 = a02 * a02 - m00 * m22, z1 = m00 * a12 - a01 * a02;  // row0 x row2
    const double x2 = m11 * m22 - a12 * a12, y2 = a12 * a02 - a01 * m22, z2 = a01 * a12 - m11 * a02;  // row1 x row2
    const double n0 = x0 * x0 + y0 * y0 + z0 * z0, n1 = x1 * x1 + y1 * y1 + z1 * z1, n2 = x2 * x2 + y2 * y2 + z2 * z2;
    double vx = x0, vy = y0, vz = z0, nn = n0;
    if (n1 > nn) vx = x1, vy = y1, vz = z1, nn = n1;
    if (n2 > nn) vx = x2, vy = y2, vz = z2, nn = n2;
    const double inv = fx_rsqrt(nn);
    vx *= inv, vy *= inv, vz *= inv;
    const double rx = m00 * vx + a01 * vy + a02 * vz, ry = a01 * vx + m11 * vy + a12 * vz, rz = a02 * vx + a12 * vy + m22 * vz;
    // The two larger eigenvalues do NOT come from the cubic: q + 2 p cos(phi -+ 2 pi / 3) contains sin(phi) = sqrt(1 - x^2), which
    // loses half the digits where two eigenvalues meet (lambda_1 ~ lambda_2, the isotropic patch: 1e-12 .. 1e-8 of lambda_2 against
    // the longdouble Jacobi, tests/test_kat_gpu.py) - and lambda_1 is the likeness, whose "near" band in fx_pca allows 1e-13.  They
    // are the eigenvalues of A restricted to the plane across v, in an orthonormal basis of it (Duff et al. 2017, branch-free): a
    // symmetric 2 x 2 problem, mean -+ hypot, every step at rounding level.  The smallest eigenvalue and its vector are what they were.
    const double sgn = copysign(1.0, vz), ia = -fx_rcp(sgn + vz), bxy = vx * vy * ia;
    const double b1x = 1.0 + sgn * vx * vx * ia, b1y = sgn * bxy, b1z = -sgn * vx;
    const double b2x = bxy, b2y = sgn + vy * vy * ia, b2z = -vy;
    const double t1x = a00 * b1x + a01 * b1y + a02 * b1z, t1y = a01 * b1x + a11 * b1y + a12 * b1z, t1z = a02 * b1x + a12 * b1y + a22 * b1z;
    const double t2x = a00 * b2x + a01 * b2y + a02 * b2z, t2y = a01 * b2x + a11 * b2y + a12 * b2z, t2z = a02 * b2x + a12 * b2y + a22 * b2z;
    const double paa = b1x * t1x + b1y * t1y + b1z * t1z, pab = b1x * t2x + b1y * t2y + b1z * t2z, pdd = b2x * t2x + b2y * t2y + b2z * t2z;
    const double hm = 0.5 * (paa + pdd), hd = 0.5 * (paa - pdd), w = hd * hd + pab * pab;
    const double rad = w > 0.0 ? w * fx_rsqrt(w) : 0.0;
    const double e1 = hm - rad, e2 = hm + rad;
    const double scale = fabs(e2) + fabs(e0);
    ok = nn > 0.0 && (rx * rx + ry * ry + rz * rz) <= 1e-24 * scale * scale && e0 <= e1 && e1 <= e2;
    if (ok) {
      ev[0] = e0, ev[1] = e1, ev[2] = e2;
      V.m[0][0] = vx, V.m[1][0] = vy, V.m[2][0] = vz;  // (only the first column is used)
      V.m[0][1] = V.m[1][1] = V.m[2][1] = V.m[0][2] = V.m[1][2] = V.m[2][2] = 0.0;
    }
  }
  if (!ok) wc::eig3_sym(A, ev, V);
  if (accepted) *accepted = ok;
}
#endif  // WC_FX_EIG3_H_
