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
// The loop of rsba_two_view_classify_pairs around them, integers and copies only:
//   homography_winner_kernel      one wave per pair over its tasks: the key (inliers + 1, 0 for a declined task) and then the lowest task that
//                                 reaches it, each by a butterfly over the wave
//   homography_pair_masks_kernel  one lane per correspondence: the inlier flag by its pair's current H
//   homography_compact_kernel     one wave per pair: the ascending inlier indices by ballot and the popcount of the lower lanes
//   homography_adopt_kernel       one lane per pair: a refit adopted iff accepted and its count is not lower; else the pair is done
// A DLT lane's result depends on its own subset only: no cross-lane operation, no atomics, no dependence on the launch geometry.
#include <climits>

#include "homography_state.hpp"
#include "hyp_math.hpp"

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

// homo_detail::invert: the adjugate over the determinant; the operations of the host form in their order, each rounded on its own (the
// inverse feeds a deciding comparison)
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

// the deciding comparison: the operations of homo_detail::transfer_inlier in their order, each rounded on its own
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
  if (A.pairs) { const HomoPair P = A.pairs[t / A.tasks_per_pair]; start = P.start; n = P.n; f2 = P.f2; }
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

// ---- the loop of rsba_two_view_classify_pairs around the kernels above: integers and copies only, so nothing here can round differently ----

__device__ __forceinline__ unsigned winner_key(const HomoWinnerArgs& A, size_t g) { return A.status[g] ? (unsigned)A.num_inliers[g] + 1u : 0u; }

__global__ __launch_bounds__(kHomoBlock) void homography_winner_kernel(const HomoWinnerArgs A) {
  const int lane = threadIdx.x, p = blockIdx.x, T = A.tasks_per_pair;
  unsigned best = 0u;
  for (int t = lane; t < T; t += kHomoBlock) best = max(best, winner_key(A, (size_t)p * T + t));
#pragma unroll
  for (int off = kHomoBlock / 2; off >= 1; off >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, off));
  int first = INT_MAX;   // the lowest task with that key
  for (int t = lane; t < T; t += kHomoBlock) first = min(first, best != 0u && winner_key(A, (size_t)p * T + t) == best ? t : INT_MAX);
#pragma unroll
  for (int off = kHomoBlock / 2; off >= 1; off >>= 1) first = min(first, __shfl_xor(first, off));
  if (lane != 0) return;
  const HomoPairState& S = A.S;
  const bool has = best != 0u;
  const int winner = has ? first : -1;
  S.status[p] = has ? 1 : 0;
  S.done[p] = has ? 0 : 1;
  S.winner_task[p] = winner;
  S.refits_adopted[p] = 0;
  S.inlier_count[p] = 0;
  const size_t g = (size_t)p * T + (has ? winner : 0);
  S.num_inliers[p] = has ? A.num_inliers[g] : 0;
  if (!has) return;
  for (int k = 0; k < 9; ++k) S.H[(size_t)p * 9 + k] = A.H[g * 9 + k];
}

__global__ __launch_bounds__(256) void homography_pair_masks_kernel(const HomoPairState S, const int32_t* __restrict__ point_pair, int first_point, int num_points,
                                                                    double thr2, const double* __restrict__ na, const double* __restrict__ nb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= num_points) return;
  const size_t g = (size_t)first_point + i;
  const int p = point_pair[g];
  if (S.done[p]) return;   // (no winner: the flags stay zero; no adopted refit: they stay the last matrix's)
  double H[9], Hi[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = S.H[(size_t)p * 9 + k];
  const bool ok = invert(H, Hi);
  S.mask[g] = ok && transfer_inlier(H, Hi, na[2 * g], na[2 * g + 1], nb[2 * g], nb[2 * g + 1], S.pairs[p].f2, thr2) ? 1 : 0;
}

// one wave per pair: lane l of a ballot writes at the running base plus the number of set lanes below it — the order of a serial push_back
__global__ __launch_bounds__(kHomoBlock) void homography_compact_kernel(const HomoPairState S) {
  const int lane = threadIdx.x, p = blockIdx.x;
  if (S.done[p]) { if (lane == 0) S.inlier_count[p] = 0; return; }   // (uniform across the wave)
  const HomoPair P = S.pairs[p];
  int count = 0;
  for (int base = 0; base < P.n; base += kHomoBlock) {   // (uniform trip count)
    const int i = base + lane;
    const bool in = i < P.n && S.mask[(size_t)P.start + i] != 0;
    const unsigned long long ballot = __ballot(in);
    if (in) S.inlier_idx[(size_t)P.start + count + __popcll(ballot & ((1ull << lane) - 1ull))] = P.start + i;
    count += __popcll(ballot);
  }
  if (lane != 0) return;
  if (count < 5) { S.done[p] = 1; count = 0; }   // (a refit takes at least five inliers; later rounds skip the pair)
  S.inlier_count[p] = count;
}

__global__ __launch_bounds__(256) void homography_adopt_kernel(const HomoAdoptArgs A) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const HomoPairState& S = A.S;
  if (p >= S.num_pairs || S.done[p]) return;
  if (!A.status[p] || A.num_inliers[p] < S.num_inliers[p]) { S.done[p] = 1; return; }   // not adopted: the next round would refit the same set
  S.num_inliers[p] = A.num_inliers[p];
  for (int k = 0; k < 9; ++k) S.H[(size_t)p * 9 + k] = A.H[(size_t)p * 9 + k];
  S.refits_adopted[p] += 1;
}

// ---- the parallax rule ----
// epi_detail::sampson_inlier / in_front, restated as kernels_epipolar.hip restates them: the host form's operations in its order
__device__ __forceinline__ bool sampson_inlier(const double E[9], double xa, double ya, double xb, double yb, double f2, double thr2) {
#pragma clang fp contract(off)
  const double l0 = E[0] * xa + E[1] * ya + E[2], l1 = E[3] * xa + E[4] * ya + E[5], l2 = E[6] * xa + E[7] * ya + E[8];
  const double m0 = E[0] * xb + E[3] * yb + E[6], m1 = E[1] * xb + E[4] * yb + E[7];
  const double r = xb * l0 + yb * l1 + l2;
  const double den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
  const double d2 = (r * r) / den;
  return d2 * f2 <= thr2;
}
__device__ __forceinline__ bool in_front(const double R[9], const double t[3], double xa, double ya, double xb, double yb) {
#pragma clang fp contract(off)
  const double p0 = R[0] * xa + R[1] * ya + R[2], p1 = R[3] * xa + R[4] * ya + R[5], p2 = R[6] * xa + R[7] * ya + R[8];
  const double t0 = 1.0 * t[0], t1 = 1.0 * t[1], t2 = 1.0 * t[2];
  const double pp = p0 * p0 + p1 * p1 + p2 * p2, qq = xb * xb + yb * yb + 1.0, pq = p0 * xb + p1 * yb + p2;
  const double pt = p0 * t0 + p1 * t1 + p2 * t2, qt = xb * t0 + yb * t1 + t2;
  const double det = pp * qq - pq * pq;
  const double za = (pq * qt - qq * pt) / det, zb = (pp * qt - pq * pt) / det;
  return za > 0.0 && zb > 0.0;
}
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
    const HomoPair P = A.pairs[p];
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
        fr = sampson_inlier(E, xa, ya, xb, yb, P.f2, A.thr2) && in_front(R, tv, xa, ya, xb, yb);
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
hipError_t launch_homography_winner(const HomoWinnerArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(homography_winner_kernel, dim3(A.S.num_pairs), dim3(kHomoBlock), 0, st, A);
  return hipGetLastError();
}
hipError_t launch_homography_pair_masks(const HomoPairState& S, const int32_t* point_pair, int first_point, int num_points, double thr2, const double* na, const double* nb,
                                        hipStream_t st) {
  if (num_points <= 0) return hipSuccess;
  hipLaunchKernelGGL(homography_pair_masks_kernel, dim3((num_points + 255) / 256), dim3(256), 0, st, S, point_pair, first_point, num_points, thr2, na, nb);
  return hipGetLastError();
}
hipError_t launch_homography_compact(const HomoPairState& S, hipStream_t st) {
  hipLaunchKernelGGL(homography_compact_kernel, dim3(S.num_pairs), dim3(kHomoBlock), 0, st, S);
  return hipGetLastError();
}
hipError_t launch_homography_adopt(const HomoAdoptArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(homography_adopt_kernel, dim3((A.S.num_pairs + 255) / 256), dim3(256), 0, st, A);
  return hipGetLastError();
}
hipError_t launch_two_view_parallax(const ParallaxArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(two_view_parallax_kernel, dim3(A.num_pairs), dim3(kHomoBlock), 0, st, A);
  return hipGetLastError();
}

}  // namespace rsba
