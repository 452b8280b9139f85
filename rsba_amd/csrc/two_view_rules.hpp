// The deciding comparisons of the two-view kernels (kernels_epipolar.hip, kernels_homography.hip, kernels_pair_loop.hip): the device
// restatement of epi_detail::sampson_inlier / in_front (include/rsba/two_view.hpp) and homo_detail::invert / transfer_inlier
// (include/rsba/pair_geometry.hpp).  The host functions are the definition: each one here has the host form's operations in the host form's
// order, each rounded on its own (contraction off), because an inlier flag or a count hangs on the last bit.  As in hyp_math.hpp, no
// anonymous namespace: a tool that includes several kernel files into one translation unit sees one definition.
#pragma once
#include <hip/hip_runtime.h>

namespace rsba {

__device__ __forceinline__ bool sampson_inlier(const double E[9], double xa, double ya, double xb, double yb, double f2, double thr2) {
#pragma clang fp contract(off)
  const double l0 = E[0] * xa + E[1] * ya + E[2], l1 = E[3] * xa + E[4] * ya + E[5], l2 = E[6] * xa + E[7] * ya + E[8];
  const double m0 = E[0] * xb + E[3] * yb + E[6], m1 = E[1] * xb + E[4] * yb + E[7];
  const double r = xb * l0 + yb * l1 + l2;
  const double den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
  const double d2 = (r * r) / den;
  return d2 * f2 <= thr2;
}

// sign: +1 or -1, the candidate's translation is sign t (the parallax rule passes 1.0: 1.0 * t is t exactly)
__device__ __forceinline__ bool in_front(const double R[9], const double t[3], double sign, double xa, double ya, double xb, double yb) {
#pragma clang fp contract(off)
  const double p0 = R[0] * xa + R[1] * ya + R[2], p1 = R[3] * xa + R[4] * ya + R[5], p2 = R[6] * xa + R[7] * ya + R[8];
  const double t0 = sign * t[0], t1 = sign * t[1], t2 = sign * t[2];
  const double pp = p0 * p0 + p1 * p1 + p2 * p2, qq = xb * xb + yb * yb + 1.0, pq = p0 * xb + p1 * yb + p2;
  const double pt = p0 * t0 + p1 * t1 + p2 * t2, qt = xb * t0 + yb * t1 + t2;
  const double det = pp * qq - pq * pq;
  const double za = (pq * qt - qq * pt) / det, zb = (pp * qt - pq * pt) / det;
  return za > 0.0 && zb > 0.0;
}

// the adjugate over the determinant (the inverse feeds transfer_inlier)
__device__ __forceinline__ bool invert(const double H[9], double Hi[9]) {
#pragma clang fp contract(off)
  const double c0 = H[4] * H[8] - H[5] * H[7], c1 = H[5] * H[6] - H[3] * H[8], c2 = H[3] * H[7] - H[4] * H[6];
  const double det = H[0] * c0 + H[1] * c1 + H[2] * c2;
  if (!(fabs(det) > 0.0)) return false;
  Hi[0] = c0 / det; Hi[1] = (H[2] * H[7] - H[1] * H[8]) / det; Hi[2] = (H[1] * H[5] - H[2] * H[4]) / det;
  Hi[3] = c1 / det; Hi[4] = (H[0] * H[8] - H[2] * H[6]) / det; Hi[5] = (H[2] * H[3] - H[0] * H[5]) / det;
  Hi[6] = c2 / det; Hi[7] = (H[1] * H[6] - H[0] * H[7]) / det; Hi[8] = (H[0] * H[4] - H[1] * H[3]) / det;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) finite = finite && isfinite(Hi[k]);
  return finite;
}

__device__ __forceinline__ bool transfer_inlier(const double H[9], const double Hi[9], double xa, double ya, double xb, double yb, double f2, double thr2) {
#pragma clang fp contract(off)
  const double w = H[6] * xa + H[7] * ya + H[8];
  if (!(w > 0.0)) return false;
  const double u = (H[0] * xa + H[1] * ya + H[2]) / w, v = (H[3] * xa + H[4] * ya + H[5]) / w;
  const double eu = xb - u, ev = yb - v;
  const double dab = eu * eu + ev * ev;
  const double w2 = Hi[6] * xb + Hi[7] * yb + Hi[8];
  if (!(w2 > 0.0)) return false;
  const double u2 = (Hi[0] * xb + Hi[1] * yb + Hi[2]) / w2, v2 = (Hi[3] * xb + Hi[4] * yb + Hi[5]) / w2;
  const double fu = xa - u2, fv = ya - v2;
  const double dba = fu * fu + fv * fv;
  const double d2 = dab > dba ? dab : dba;
  return d2 * f2 <= thr2;
}

}  // namespace rsba
