// Essential-matrix hypotheses of the two-view bootstrap (include/rsba/two_view.hpp: epi_detail::eight_point, decompose, score and what they
// call — hartley, null_matrix, essential_svd, sampson_inlier, in_front, hyp_detail::eigen3, smallest_eigenvector12, pose_from_rt), for every
// subset at once.  The host functions are the definition; this file restates them for the device, fp64 throughout, every loop with the
// host's fixed bound (60 / 40 Jacobi sweeps).
//   epipolar_eight_point_kernel  one lane per subset, one wave per workgroup.  The 9 x 9 Gram matrix (lower triangle, 45 entries) and the
//                                81 entries of the accumulated rotations live in LDS, lane-interleaved as pnp_dlt_kernel keeps its own
//                                (entry e of lane l at [e][l]: conflict-free, and indexable by the run-time (p, q) of a Jacobi rotation).
//                                126 x 64 doubles = 64 512 bytes per workgroup: within a default launch.  The host's three idle unknowns are
//                                never rotated (their off-diagonals are zero), so they appear here only as the value 2 trace in the gap test.
//                                The rotation is applied in its symmetric form, as in pnp_dlt_kernel: the same angles, another operation order.
//                                The 3 x 3 work is unrolled in registers.
//   epipolar_score_kernel        one wave per hypothesis: every lane holds the decomposition of the hypothesis (computed once, before the
//                                loop), the lanes stride over the correspondences, the five counts are sums of ballot popcounts — integers,
//                                so lane order cannot matter.  Lane 0 writes the counts and the winning candidate's pose.
//   epipolar_inliers_kernel      one lane per correspondence: the inlier flags of one E
// The RANSAC of many frame pairs in one call (rsba_epipolar_ransac_pairs) runs the two kernels above over the concatenated points of all
// pairs — the eight-point kernel with an optional list per task (the refits, one lane per pair), the score kernel with an optional pair
// table (a task counts over its pair's range with its pair's focal length) — so that a pair's numbers are rounded by the code that rounds
// them in the single-pair calls.  The loop around them (winner, masks, compaction, adopt) is kernels_pair_loop.hip, shared with the
// homography; the two deciding comparisons, sampson_inlier and in_front, are two_view_rules.hpp's.
// An eight-point lane's result depends on its own subset only: no cross-lane operation, no atomics, no dependence on the launch geometry.
#include "epipolar_state.hpp"
#include "hyp_math.hpp"
#include "two_view_rules.hpp"

namespace rsba {

namespace {

constexpr int kEpiBlock = 64;                 // one wave per workgroup
constexpr int kTri = 45;                      // lower triangle of 9 x 9
constexpr int kVec = 81;                      // the eigenvector matrix

// epi_detail::essential_svd: U, V as [column][row]
__device__ __forceinline__ bool essential_svd(const double E[9], double U[3][3], double V[3][3], double s[2]) {
  double sm[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    sm[0] += E[3 * r] * E[3 * r]; sm[1] += E[3 * r] * E[3 * r + 1]; sm[2] += E[3 * r] * E[3 * r + 2];
    sm[3] += E[3 * r + 1] * E[3 * r + 1]; sm[4] += E[3 * r + 1] * E[3 * r + 2]; sm[5] += E[3 * r + 2] * E[3 * r + 2];
  }
  double val[3], vec[3][3];
  eigen3(sm, val, vec);
  s[0] = sqrt(fmax(0.0, val[2])); s[1] = sqrt(fmax(0.0, val[1]));
  if (!(s[1] > 1e-6 * s[0])) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) { V[0][k] = vec[k][2]; V[1][k] = vec[k][1]; }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
#pragma unroll
    for (int r = 0; r < 3; ++r) U[c][r] = (E[3 * r] * V[c][0] + E[3 * r + 1] * V[c][1] + E[3 * r + 2] * V[c][2]) / s[c];
  }
  U[2][0] = U[0][1] * U[1][2] - U[0][2] * U[1][1]; U[2][1] = U[0][2] * U[1][0] - U[0][0] * U[1][2]; U[2][2] = U[0][0] * U[1][1] - U[0][1] * U[1][0];
  V[2][0] = V[0][1] * V[1][2] - V[0][2] * V[1][1]; V[2][1] = V[0][2] * V[1][0] - V[0][0] * V[1][2]; V[2][2] = V[0][0] * V[1][1] - V[0][1] * V[1][0];
  // which way round (v1, v2) runs in their plane: the largest component of v3 (the first such) positive
  double lead = V[2][0];
#pragma unroll
  for (int k = 1; k < 3; ++k) if (fabs(V[2][k]) > fabs(lead)) lead = V[2][k];
  if (lead < 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { V[1][k] = -V[1][k]; U[1][k] = -U[1][k]; V[2][k] = -V[2][k]; U[2][k] = -U[2][k]; }
  }
  return true;
}

__global__ __launch_bounds__(kEpiBlock) void epipolar_eight_point_kernel(const EpiEightArgs A) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x, t = blockIdx.x * kEpiBlock + lane;
  if (t >= A.num_tasks) return;                  // (no barrier anywhere below)
  double* G = smem + lane;                       // G[e * 64]: Gram matrix, lower triangle
  double* V = smem + kTri * kEpiBlock + lane;    // V[(k * 9 + col) * 64]
  // a fixed m per task, or (the refits of rsba_epipolar_ransac_pairs) a list per task: one kernel for both, so that both round alike
  const int m = A.sub_start ? A.sub_count[t] : A.m;
  const int32_t* sub = A.subsets + (A.sub_start ? (size_t)A.sub_start[t] : (size_t)t * A.m);
  const double* na = A.na;
  const double* nb = A.nb;
  A.status[t] = 0;
  if (m < 8) return;
  for (int i = 0; i < m; ++i) for (int k = i + 1; k < m; ++k) if (sub[i] == sub[k]) return;

  // ---- hartley ----
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

  // ---- null_matrix: the Gram matrix of one row per point ----
  for (int e = 0; e < kTri; ++e) G[e * kEpiBlock] = 0.0;
  for (int i = 0; i < m; ++i) {
    const size_t j = 2 * (size_t)sub[i];
    const double xa = (na[j] - ca0) / sa, ya = (na[j + 1] - ca1) / sa, xb = (nb[j] - cb0) / sb, yb = (nb[j + 1] - cb1) / sb;
    const double r[9] = {xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, 1.0};
#pragma unroll
    for (int a = 0; a < 9; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) G[(a * (a + 1) / 2 + b) * kEpiBlock] += r[a] * r[b];
    }
  }
  double big = 0.0;
  for (int a = 0; a < 9; ++a) big += G[sym(a, a) * kEpiBlock];
  if (!(big > 0.0)) return;

  // ---- smallest_eigenvector12 on its 9 active unknowns (2 big: the idle unknowns' eigenvalue): cyclic Jacobi on the triangle in LDS ----
  const int best = smallest_eigenvector_lds<9, kEpiBlock>(G, V, 2.0 * big);
  if (best < 0) return;                          // a second null direction: a plane, or no baseline
  double ev[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) ev[k] = V[(k * 9 + best) * kEpiBlock];

  // ---- the normalisation undone, the projection onto the essential manifold, the sign ----
  double M[9], F[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    M[3 * r] = ev[3 * r] / sa; M[3 * r + 1] = ev[3 * r + 1] / sa;
    M[3 * r + 2] = ev[3 * r + 2] - (ca0 * ev[3 * r] + ca1 * ev[3 * r + 1]) / sa;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    F[k] = M[k] / sb; F[3 + k] = M[3 + k] / sb;
    F[6 + k] = M[6 + k] - (cb0 * M[k] + cb1 * M[3 + k]) / sb;
  }
  double U[3][3], W[3][3], s[2], out[9];
  if (!essential_svd(F, U, W, s)) return;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * r + k] = U[0][r] * W[0][k] + U[1][r] * W[1][k];
  }
  double lead = out[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) if (fabs(out[k]) > fabs(lead)) lead = out[k];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) { if (lead < 0) out[k] = -out[k]; finite = finite && isfinite(out[k]); }
  if (!finite) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) A.E_out[(size_t)t * 9 + k] = out[k];
  A.status[t] = 1;
}

__global__ __launch_bounds__(kEpiBlock) void epipolar_score_kernel(const EpiScoreArgs A) {
  const int lane = threadIdx.x, t = blockIdx.x;   // (one workgroup per task: every branch on t is uniform across the wave)
  const bool skip = A.status_in && A.status_in[t] == 0;
  double E[9], R[2][9], tv[3];
  bool ok = !skip;
  if (ok) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = A.E[(size_t)t * 9 + k];
    // ---- epi_detail::decompose ----
    double U[3][3], V[3][3], s[2];
    ok = essential_svd(E, U, V, s);
    if (ok) {
      const double nt = sqrt(U[2][0] * U[2][0] + U[2][1] * U[2][1] + U[2][2] * U[2][2]);
      ok = nt > 0.0;
      bool finite = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) tv[k] = U[2][k] / nt;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double w = U[1][r] * V[0][k] - U[0][r] * V[1][k], z = U[2][r] * V[2][k];
          R[0][3 * r + k] = w + z; R[1][3 * r + k] = z - w;
          finite = finite && isfinite(w + z) && isfinite(z - w);
        }
      }
      ok = ok && finite && isfinite(tv[0] + tv[1] + tv[2]);
    }
  }
  // the correspondences the task counts over: all of them, or (a batched call) the range of the task's pair, with the pair's focal length
  int start = 0, n = A.n;
  double f2 = A.f2;
  if (A.pairs) { const PairRange P = A.pairs[t / A.tasks_per_pair]; start = P.start; n = P.n; f2 = P.f2; }
  int inl = 0, front[4] = {0, 0, 0, 0};
  if (ok) {
    for (int base = 0; base < n; base += kEpiBlock) {   // (uniform trip count: every lane reaches every ballot)
      const int i = base + lane;
      bool in = false, fr[4] = {false, false, false, false};
      if (i < n) {
        const size_t j = 2 * ((size_t)start + i);
        const double xa = A.na[j], ya = A.na[j + 1], xb = A.nb[j], yb = A.nb[j + 1];
        in = sampson_inlier(E, xa, ya, xb, yb, f2, A.thr2);
        if (in) {
#pragma unroll
          for (int c = 0; c < 4; ++c) fr[c] = in_front(R[c >> 1], tv, (c & 1) ? -1.0 : 1.0, xa, ya, xb, yb);
        }
      }
      inl += __popcll(__ballot(in));
#pragma unroll
      for (int c = 0; c < 4; ++c) front[c] += __popcll(__ballot(fr[c]));
    }
  }
  if (lane != 0) return;
  double pose[6];
  int best = 0;
  if (ok) {
#pragma unroll
    for (int c = 1; c < 4; ++c) if (front[c] > front[best]) best = c;
    const double sg = (best & 1) ? -1.0 : 1.0;
    const double tb[3] = {sg * tv[0], sg * tv[1], sg * tv[2]};
    double Rb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rb[k] = (best >> 1) ? R[1][k] : R[0][k];
    ok = pose_from_rt(Rb, tb, pose);
  }
  A.status[t] = ok ? 1 : 0;
  A.num_inliers[t] = ok ? inl : 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) A.num_front[(size_t)t * 4 + c] = ok ? front[c] : 0;
  if (ok) {
#pragma unroll
    for (int k = 0; k < 6; ++k) A.poses_out[(size_t)t * 6 + k] = pose[k];
  }
}

__global__ __launch_bounds__(256) void epipolar_inliers_kernel(const EpiScoreArgs A, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  double E[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = A.E[k];
  mask[i] = sampson_inlier(E, A.na[2 * (size_t)i], A.na[2 * (size_t)i + 1], A.nb[2 * (size_t)i], A.nb[2 * (size_t)i + 1], A.f2, A.thr2) ? 1 : 0;
}

}  // namespace

hipError_t launch_epipolar_eight_point(const EpiEightArgs& A, hipStream_t st) {
  const size_t lds = (size_t)(kTri + kVec) * kEpiBlock * sizeof(double);   // 64 512 bytes
  hipLaunchKernelGGL(epipolar_eight_point_kernel, dim3((A.num_tasks + kEpiBlock - 1) / kEpiBlock), dim3(kEpiBlock), lds, st, A);
  return hipGetLastError();
}
hipError_t launch_epipolar_score(const EpiScoreArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(epipolar_score_kernel, dim3(A.num_tasks), dim3(kEpiBlock), 0, st, A);
  return hipGetLastError();
}
hipError_t launch_epipolar_inliers(const EpiScoreArgs& A, uint8_t* mask, hipStream_t st) {
  hipLaunchKernelGGL(epipolar_inliers_kernel, dim3((A.n + 255) / 256), dim3(256), 0, st, A, mask);
  return hipGetLastError();
}

}  // namespace rsba
