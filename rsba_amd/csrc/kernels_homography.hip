// Homography hypotheses and the parallax counts of the two-view degeneracy test (include/rsba/pair_geometry.hpp: homo_detail::dlt, invert,
// transfer_inlier, score, parallax_counts and what they call — hyp_detail::hartley_side, null_vector9, from_pose, rotate, epi_detail::
// sampson_inlier, in_front), for every subset and every frame pair at once.  The host functions are the definition; this file restates them
// for the device, fp64 throughout, every loop with the host's fixed bound (60 Jacobi sweeps).
//   homography_dlt_kernel       one lane per subset, one wave per workgroup.  The 9 x 9 Gram matrix (lower triangle, 45 entries) and the 81
//                               entries of the accumulated rotations live in LDS, lane-interleaved as epipolar_eight_point_kernel keeps its own:
//                               126 x 64 doubles = 64 512 bytes per workgroup.  Two rows per point, (-a', 0, xb' a') and (0, -a', yb' a'); their
//                               structural zeros are not multiplied out.  `largest` starts at twice the trace, as the eight-point kernel takes it.
//                               A fixed m per task or a list per task (the refits of rsba_two_view_classify_pairs): one kernel for both.
//   homography_score_kernel     one wave per matrix: every lane holds H and its inverse (computed once, before the loop), the lanes stride over
//                               the correspondences, the count is a sum of ballot popcounts — integers, so lane order cannot matter.
//   homography_inliers_kernel   one lane per correspondence: the inlier flags of one H
//   two_view_parallax_kernel    one wave per pair: every lane holds (R, t) of the pair's pose, the lanes stride over the pair's correspondences,
//                               num_front and num_parallax are sums of ballot popcounts.
// The loop of rsba_two_view_classify_pairs around them (winner, masks, compaction, adopt) is kernels_pair_loop.hip, shared with the essential
// matrix; the deciding comparisons (invert, transfer_inlier, sampson_inlier, in_front) are two_view_rules.hpp's.
// A DLT lane's result depends on its own subset only: no cross-lane operation, no atomics, no dependence on the launch geometry.
#include "homography_state.hpp"
#include "hyp_math.hpp"
#include "two_view_rules.hpp"

namespace rsba {

namespace {

constexpr int kHomoBlock = 64;                // one wave per workgroup
constexpr int kTri = 45;                      // lower triangle of 9 x 9
constexpr int kVec = 81;                      // the eigenvector matrix

__device__ __forceinline__ double det3(const double R[9]) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

__global__ __launch_bounds__(kHomoBlock) void homography_dlt_kernel(const HomoDltArgs A) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x, t = blockIdx.x * kHomoBlock + lane;
  if (t >= A.num_tasks) return;                  // (no barrier anywhere below)
  double* G = smem + lane;                       // G[e * 64]: Gram matrix, lower triangle
  double* V = smem + kTri * kHomoBlock + lane;   // V[(k * 9 + col) * 64]
  const int m = A.sub_start ? A.sub_count[t] : A.m;
  const int32_t* sub = A.subsets + (A.sub_start ? (size_t)A.sub_start[t] : (size_t)t * A.m);
  const double* na = A.na;
  const double* nb = A.nb;
  A.status[t] = 0;
  if (m < 4) return;
  for (int i = 0; i < m; ++i) for (int k = i + 1; k < m; ++k) if (sub[i] == sub[k]) return;

  // ---- hartley_side, both sides ----
  double ca0 = 0.0, ca1 = 0.0, cb0 = 0.0, cb1 = 0.0, sa = 0.0, sb = 0.0;
  for (int i = 0; i < m; ++i) {
    const size_t j = 2 * (size_t)sub[i];
    ca0 += na[j] / m; ca1 += na[j + 1] / m; cb0 += nb[j] / m; cb1 += nb[j + 1] / m;
  }
  for (int i = 0; i < m; ++i) {
    const size_t j = 2 * (size_t)sub[i];
    sa += hypot(na[j] - ca0, na[j + 1] - ca1) / m; sb += hypot(nb[j] - cb0, nb[j + 1] - cb1) / m;
  }
  if (!(sa > 0.0) || !(sb > 0.0)) return;
  sa /= 1.4142135623730951; sb /= 1.4142135623730951;

  // ---- the Gram matrix of two rows per point; a row's three structural zeros are left out (they add nothing to a finite sum) ----
  for (int e = 0; e < kTri; ++e) G[e * kHomoBlock] = 0.0;
  for (int i = 0; i < m; ++i) {
    const size_t j = 2 * (size_t)sub[i];
    const double xa = (na[j] - ca0) / sa, ya = (na[j + 1] - ca1) / sa, xb = (nb[j] - cb0) / sb, yb = (nb[j + 1] - cb1) / sb;
    const double r1[6] = {-xa, -ya, -1.0, xb * xa, xb * ya, xb};   // unknowns 0 1 2 6 7 8
    const double r2[6] = {-xa, -ya, -1.0, yb * xa, yb * ya, yb};   // unknowns 3 4 5 6 7 8
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        const int ua = a < 3 ? a : a + 3, ub = b < 3 ? b : b + 3;
        G[(ua * (ua + 1) / 2 + ub) * kHomoBlock] += r1[a] * r1[b];
      }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        const int ua = a + 3, ub = b + 3;
        G[(ua * (ua + 1) / 2 + ub) * kHomoBlock] += r2[a] * r2[b];
      }
    }
  }
  double big = 0.0;
  for (int a = 0; a < 9; ++a) big += G[sym(a, a) * kHomoBlock];
  if (!(big > 0.0)) return;

  const int best = smallest_eigenvector_lds<9, kHomoBlock>(G, V, 2.0 * big);
  if (best < 0) return;                          // a second null direction: three of the four points on a line, coincident points
  double ev[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) ev[k] = V[(k * 9 + best) * kHomoBlock];

  // ---- the normalisation undone (H = Tb^-1 Hn Ta), unit Frobenius norm, the sign, the last reasons to decline ----
  double M[9], H[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    M[3 * r] = ev[3 * r] / sa; M[3 * r + 1] = ev[3 * r + 1] / sa;
    M[3 * r + 2] = ev[3 * r + 2] - (ca0 * ev[3 * r] + ca1 * ev[3 * r + 1]) / sa;
  }
  double fro = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    H[k] = sb * M[k] + cb0 * M[6 + k]; H[3 + k] = sb * M[3 + k] + cb1 * M[6 + k]; H[6 + k] = M[6 + k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) fro += H[k] * H[k];
  fro = sqrt(fro);
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] /= fro;
  {
    const size_t j = 2 * (size_t)sub[0];
    const double z0 = H[6] * na[j] + H[7] * na[j + 1] + H[8];
    if (z0 < 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) H[k] = -H[k];
    }
  }
  for (int i = 0; i < m; ++i) {                  // the orientation test: every point of the subset in front of the plane at infinity's image
    const size_t j = 2 * (size_t)sub[i];
    if (!(H[6] * na[j] + H[7] * na[j + 1] + H[8] > 0.0)) return;
  }
  if (!(fabs(det3(H)) > 1e-6)) return;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) finite = finite && isfinite(H[k]);
  if (!finite) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) A.H_out[(size_t)t * 9 + k] = H[k];
  A.status[t] = 1;
}

__global__ __launch_bounds__(kHomoBlock) void homography_score_kernel(const HomoScoreArgs A) {
  const int lane = threadIdx.x, t = blockIdx.x;   // (one workgroup per task: every branch on t is uniform across the wave)
  double H[9], Hi[9];
  bool ok = !(A.status_in && A.status_in[t] == 0);
  if (ok) {
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = A.H[(size_t)t * 9 + k];
    ok = invert(H, Hi);
  }
  int start = 0, n = A.n;
  double f2 = A.f2;
  if (A.pairs) { const PairRange P = A.pairs[t / A.tasks_per_pair]; start = P.start; n = P.n; f2 = P.f2; }
  int inl = 0;
  if (ok) {
    for (int base = 0; base < n; base += kHomoBlock) {   // (uniform trip count: every lane reaches every ballot)
      const int i = base + lane;
      bool in = false;
      if (i < n) {
        const size_t j = 2 * ((size_t)start + i);
        in = transfer_inlier(H, Hi, A.na[j], A.na[j + 1], A.nb[j], A.nb[j + 1], f2, A.thr2);
      }
      inl += __popcll(__ballot(in));
    }
  }
  if (lane != 0) return;
  A.status[t] = ok ? 1 : 0;
  A.num_inliers[t] = ok ? inl : 0;
}

__global__ __launch_bounds__(256) void homography_inliers_kernel(const HomoScoreArgs A, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  double H[9], Hi[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = A.H[k];
  const bool ok = invert(H, Hi);
  mask[i] = ok && transfer_inlier(H, Hi, A.na[2 * (size_t)i], A.na[2 * (size_t)i + 1], A.nb[2 * (size_t)i], A.nb[2 * (size_t)i + 1], A.f2, A.thr2) ? 1 : 0;
}

// ---- the parallax rule ----
// the angle between the rays a and R^T b is at least the threshold: a . (R^T b) <= c sqrt(|a|^2 |R^T b|^2)
__device__ __forceinline__ bool has_parallax(const double R[9], double xa, double ya, double xb, double yb, double c) {
#pragma clang fp contract(off)
  const double q0 = R[0] * xb + R[3] * yb + R[6], q1 = R[1] * xb + R[4] * yb + R[7], q2 = R[2] * xb + R[5] * yb + R[8];
  const double dot = xa * q0 + ya * q1 + q2;
  const double aa = xa * xa + ya * ya + 1.0, qq = q0 * q0 + q1 * q1 + q2 * q2;
  return dot <= c * sqrt(aa * qq);
}

__global__ __launch_bounds__(kHomoBlock) void two_view_parallax_kernel(const ParallaxArgs A) {
  const int lane = threadIdx.x, p = blockIdx.x;   // (one workgroup per pair: every branch on p is uniform across the wave)
  int front = 0, par = 0;
  if (A.pair_status[p]) {
    const PairRange P = A.pairs[p];
    double E[9], R[9], tv[3], pose[6];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = A.E[(size_t)p * 9 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) pose[k] = A.poses[(size_t)p * 6 + k];
    // homo_detail::pose_rt: column k of R is the rotated unit vector k, t = -R centre
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
      double r[3];
      rotate(pose, e, r);
      R[k] = r[0]; R[3 + k] = r[1]; R[6 + k] = r[2];
    }
    {
      double r[3];
      rotate(pose, pose + 3, r);
      tv[0] = -r[0]; tv[1] = -r[1]; tv[2] = -r[2];
    }
    for (int base = 0; base < P.n; base += kHomoBlock) {   // (uniform trip count: every lane reaches every ballot)
      const int i = base + lane;
      bool fr = false, pa = false;
      if (i < P.n) {
        const size_t j = 2 * ((size_t)P.start + i);
        const double xa = A.na[j], ya = A.na[j + 1], xb = A.nb[j], yb = A.nb[j + 1];
        fr = sampson_inlier(E, xa, ya, xb, yb, P.f2, A.thr2) && in_front(R, tv, 1.0, xa, ya, xb, yb);
        pa = fr && has_parallax(R, xa, ya, xb, yb, A.cos_min);
      }
      front += __popcll(__ballot(fr));
      par += __popcll(__ballot(pa));
    }
  }
  if (lane != 0) return;
  A.num_front[p] = front;
  A.num_parallax[p] = par;
}

}  // namespace

hipError_t launch_homography_dlt(const HomoDltArgs& A, hipStream_t st) {
  const size_t lds = (size_t)(kTri + kVec) * kHomoBlock * sizeof(double);   // 64 512 bytes
  hipLaunchKernelGGL(homography_dlt_kernel, dim3((A.num_tasks + kHomoBlock - 1) / kHomoBlock), dim3(kHomoBlock), lds, st, A);
  return hipGetLastError();
}
hipError_t launch_homography_score(const HomoScoreArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(homography_score_kernel, dim3(A.num_tasks), dim3(kHomoBlock), 0, st, A);
  return hipGetLastError();
}
hipError_t launch_homography_inliers(const HomoScoreArgs& A, uint8_t* mask, hipStream_t st) {
  hipLaunchKernelGGL(homography_inliers_kernel, dim3((A.n + 255) / 256), dim3(256), 0, st, A, mask);
  return hipGetLastError();
}
hipError_t launch_two_view_parallax(const ParallaxArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(two_view_parallax_kernel, dim3(A.num_pairs), dim3(kHomoBlock), 0, st, A);
  return hipGetLastError();
}

}  // namespace rsba
