// The five-point solver of the two-view bootstrap (include/rsba_amd.h: rsba_epipolar_five_point; include/rsba/two_view.hpp:
// epi_detail::five_point and what it calls — fp_null_space, fp_constraints, fp_eliminate, fp_reduce, fp_eliminant, fp_roots_unit, hyp_detail::poly_bisect,
// fp_polish, fp_solution, fp_key), for every subset at once.  The host functions are the definition; this file restates them for the
// device, fp64 throughout, every loop with the host's fixed bound, and — the whole file — without contraction: every product and sum is
// rounded on its own, in the host's order, so the pivots, the brackets of the roots, the minor that gives (x, y), the sign and the order
// of the solutions are decided on the numbers the host decides them on.
//   epipolar_five_point_kernel  one lane per subset.  Everything a lane indexes at run time lives in LDS, lane-interleaved (entry e of lane l
//                               at [e][l]: conflict-free): first the five constraint rows and their Householder vectors, then the 10 x 20
//                               matrix (200 doubles) beside the null-space basis (36), then — in the matrix's place, of which only rows 4..9
//                               are read after the elimination — B(z), the ladder of derivatives, the brackets, the solutions and their
//                               keys.  258 doubles per lane.  What is indexed at compile time after unrolling (the polynomial products of
//                               the cubics, the eliminant, the polish) is in registers.
//                               kFiveLanes subsets per workgroup: see launch_epipolar_five_point.
//   epipolar_pick_kernel        one lane per subset: of its ten scored slots the one with the most inliers, ties to the most in front,
//                               then to the first (epi_detail::five_point_hypothesis)
// A lane's result depends on its own subset only: no cross-lane operation, no atomics, no dependence on the launch geometry.
#include "epipolar_state.hpp"

#pragma clang fp contract(off)

namespace rsba {

namespace {

#ifndef RSBA_FIVE_LANES
#define RSBA_FIVE_LANES 64
#endif
constexpr int kFiveLanes = RSBA_FIVE_LANES;   // subsets per workgroup: one wave (32 would leave half of it idle)
constexpr double kFiveRankTol = 1e-7, kFivePivotTol = 1e-7;
constexpr int kFiveBisections = 40, kFiveNewton = 2, kFivePolish = 2;
// offsets into a lane's LDS, in doubles
constexpr int kOffRows = 0, kOffBeta = 45;                 // until the null space is known
constexpr int kOffM = 0, kOffN = 222;                      // the 10 x 20 matrix; the basis N[4][9] (to the end)
constexpr int kOffB = 0, kOffLadder = 45, kOffEdge = 110, kOffSol = 122, kOffKey = 212;   // after the elimination (rows 4..9 of M: 80..199, read before the ladder is written)
constexpr int kFiveDoubles = 258;

__device__ __forceinline__ constexpr int quad_index(int i, int j) { return i <= j ? i * 4 - i * (i - 1) / 2 + (j - i) : j * 4 - j * (j - 1) / 2 + (i - j); }

// q += s a b, c += s q l: epi_detail::fp_quad_add / fp_cubic_add, every index a constant after unrolling
__device__ __forceinline__ void quad_add(double q[10], const double a[4], const double b[4], double s) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) q[quad_index(i, j)] += s * (a[i] * b[j]);
  }
}
__device__ __forceinline__ void cubic_add(double c[20], const double q[10], const double l[4], double s) {
  constexpr int kCubic[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {5, 9, 11, 12}, {3, 1, 6, 7},
                                 {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
#pragma unroll
  for (int k = 0; k < 10; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[kCubic[k][j]] += s * (q[k] * l[j]);
  }
}

template <int LANES>
struct Lane {
  double* S;   // this lane's column of the workgroup's LDS
  __device__ __forceinline__ double& operator()(int e) const { return S[e * LANES]; }
  // hyp_detail::poly_eval on coefficients at offset c
  __device__ __forceinline__ double eval(int c, int deg, double t) const {
    double h = (*this)(c + deg);
#pragma unroll 1
    for (int k = deg - 1; k >= 0; --k) h = h * t + (*this)(c + k);
    return h;
  }
  // hyp_detail::poly_bisect
  __device__ __forceinline__ bool bisect(int c, int deg, double lo, double hi, double* root) const {
    *root = hi;
    const bool plo = eval(c, deg, lo) > 0.0, phi = eval(c, deg, hi) > 0.0;
    if (plo == phi) return false;
#pragma unroll 1
    for (int it = 0; it < kFiveBisections; ++it) {
      const double mid = 0.5 * (lo + hi);
      if ((eval(c, deg, mid) > 0.0) == plo) lo = mid; else hi = mid;
    }
    *root = 0.5 * (lo + hi);
    return true;
  }
};

__device__ __forceinline__ constexpr int ladder(int d) { return kOffLadder + d * (d + 1) / 2 - 1; }   // the d + 1 coefficients of the derivative of degree d

// epi_detail::fp_polish
__device__ __forceinline__ void polish(const double N[4][9], double v[3]) {
#pragma unroll 1
  for (int it = 0; it < kFivePolish; ++it) {
    double E[9], G[3][3], r[10], J[10][3];
#pragma unroll
    for (int m = 0; m < 9; ++m) E[m] = v[0] * N[0][m] + v[1] * N[1][m] + v[2] * N[2][m] + N[3][m];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) G[i][j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
    }
    const double tr = G[0][0] + G[1][1] + G[2][2];
    const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                           E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                           E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
    r[0] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) r[1 + 3 * i + c] = 2.0 * (G[i][0] * E[c] + G[i][1] * E[3 + c] + G[i][2] * E[6 + c]) - tr * E[3 * i + c];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double* D = N[d];
      double dG[3][3], dtr = 0.0, dd = 0.0;
#pragma unroll
      for (int m = 0; m < 9; ++m) { dtr += E[m] * D[m]; dd += cof[m] * D[m]; }
      dtr *= 2.0;
      J[0][d] = dd;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
          dG[i][j] = D[3 * i] * E[3 * j] + D[3 * i + 1] * E[3 * j + 1] + D[3 * i + 2] * E[3 * j + 2] + E[3 * i] * D[3 * j] + E[3 * i + 1] * D[3 * j + 1] + E[3 * i + 2] * D[3 * j + 2];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          J[1 + 3 * i + c][d] = 2.0 * (dG[i][0] * E[c] + dG[i][1] * E[3 + c] + dG[i][2] * E[6 + c] + G[i][0] * D[c] + G[i][1] * D[3 + c] + G[i][2] * D[6 + c])
                                - dtr * E[3 * i + c] - tr * D[3 * i + c];
      }
    }
    double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      A[0] += J[k][0] * J[k][0]; A[1] += J[k][0] * J[k][1]; A[2] += J[k][0] * J[k][2]; A[3] += J[k][1] * J[k][1]; A[4] += J[k][1] * J[k][2]; A[5] += J[k][2] * J[k][2];
      b[0] += J[k][0] * r[k]; b[1] += J[k][1] * r[k]; b[2] += J[k][2] * r[k];
    }
    const double c00 = A[3] * A[5] - A[4] * A[4], c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3];
    const double c11 = A[0] * A[5] - A[2] * A[2], c12 = A[1] * A[2] - A[0] * A[4], c22 = A[0] * A[3] - A[1] * A[1];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    const double s0 = (c00 * b[0] + c01 * b[1] + c02 * b[2]) / det, s1 = (c01 * b[0] + c11 * b[1] + c12 * b[2]) / det, s2 = (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det;
    if (!isfinite(s0 + s1 + s2)) return;
    v[0] -= s0; v[1] -= s1; v[2] -= s2;
  }
}

// epi_detail::fp_solution into slot `slot` of the lane's solutions, with its key; false: not finite
template <int LANES>
__device__ __forceinline__ bool solution(const Lane<LANES>& L, double z, int slot) {
  double b[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int v = 0; v < 3; ++v) b[r][v] = L.eval(kOffB + (r * 3 + v) * 5, 4, z);
  }
  const double C[3] = {b[1][0] * b[2][1] - b[2][0] * b[1][1], b[2][0] * b[0][1] - b[0][0] * b[2][1], b[0][0] * b[1][1] - b[1][0] * b[0][1]};
  int k = 0;
  if (fabs(C[1]) > fabs(C[0])) k = 1;
  if (fabs(C[2]) > fabs(k == 1 ? C[1] : C[0])) k = 2;
  double v[3];
  if (k == 0) { v[0] = (b[1][1] * b[2][2] - b[1][2] * b[2][1]) / C[0]; v[1] = (b[1][2] * b[2][0] - b[1][0] * b[2][2]) / C[0]; }
  else if (k == 1) { v[0] = (b[2][1] * b[0][2] - b[2][2] * b[0][1]) / C[1]; v[1] = (b[2][2] * b[0][0] - b[2][0] * b[0][2]) / C[1]; }
  else { v[0] = (b[0][1] * b[1][2] - b[0][2] * b[1][1]) / C[2]; v[1] = (b[0][2] * b[1][0] - b[0][0] * b[1][2]) / C[2]; }
  v[2] = z;
  double N[4][9];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int i = 0; i < 9; ++i) N[m][i] = L(kOffN + m * 9 + i);
  }
  polish(N, v);
  double E[9], fro = 0.0;
#pragma unroll
  for (int m = 0; m < 9; ++m) { E[m] = v[0] * N[0][m] + v[1] * N[1][m] + v[2] * N[2][m] + N[3][m]; fro += E[m] * E[m]; }
  fro = sqrt(fro);
#pragma unroll
  for (int m = 0; m < 9; ++m) E[m] /= fro;
  double lead = E[0];
#pragma unroll
  for (int m = 1; m < 9; ++m) if (fabs(E[m]) > fabs(lead)) lead = E[m];
  bool finite = true;
  double key = 0.0;
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    if (lead < 0) E[m] = -E[m];
    finite = finite && isfinite(E[m]);
    key += (m + 1) * E[m];
    L(kOffSol + slot * 9 + m) = E[m];
  }
  L(kOffKey + slot) = fabs(key);
  return finite;
}

template <int LANES>
__global__ __launch_bounds__(LANES) void epipolar_five_point_kernel(const EpiFiveArgs A) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x, t = blockIdx.x * LANES + lane;
  if (t >= A.num_tasks) return;                  // (no barrier anywhere below)
  const Lane<LANES> L{smem + lane};
  const double* na = A.na;
  const double* nb = A.nb;
  const int32_t* sub = A.subsets + (size_t)t * 5;
  A.status[t] = 0;
  A.num_solutions[t] = 0;
  for (int s = 0; s < 10; ++s) A.slot_status[(size_t)t * 10 + s] = 0;
  for (int i = 0; i < 5; ++i) for (int k = i + 1; k < 5; ++k) if (sub[i] == sub[k]) return;

  // ---- fp_null_space: the constraint rows, five Householder reflections, the basis ----
#pragma unroll 1
  for (int i = 0; i < 5; ++i) {
    const size_t j = 2 * (size_t)sub[i];
    const double xa = na[j], ya = na[j + 1], xb = nb[j], yb = nb[j + 1];
    const double r[9] = {xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, 1.0};
#pragma unroll
    for (int k = 0; k < 9; ++k) L(kOffRows + i * 9 + k) = r[k];
  }
  double longest = 0.0;
#pragma unroll 1
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
    for (int i = 0; i < 9; ++i) { const double a = L(kOffRows + k * 9 + i); s += a * a; }
    longest = fmax(longest, sqrt(s));
  }
#pragma unroll 1
  for (int k = 0; k < 5; ++k) {
    const int row = kOffRows + k * 9;
    double s = 0.0;
    for (int i = k; i < 9; ++i) { const double a = L(row + i); s += a * a; }
    const double nrm = sqrt(s);
    if (!(nrm > kFiveRankTol * longest)) return;   // a fifth null direction
    const double akk = L(row + k);
    L(row + k) = akk - (akk >= 0.0 ? -nrm : nrm);
    double vv = 0.0;
    for (int i = k; i < 9; ++i) { const double a = L(row + i); vv += a * a; }
    const double beta = 2.0 / vv;
    L(kOffBeta + k) = beta;
#pragma unroll 1
    for (int j = k + 1; j < 5; ++j) {
      const int other = kOffRows + j * 9;
      double d = 0.0;
      for (int i = k; i < 9; ++i) d += L(row + i) * L(other + i);
      d *= beta;
      for (int i = k; i < 9; ++i) L(other + i) -= d * L(row + i);
    }
  }
#pragma unroll 1
  for (int m = 0; m < 4; ++m) {
    const int vec = kOffN + m * 9;
    for (int i = 0; i < 9; ++i) L(vec + i) = i == 5 + m ? 1.0 : 0.0;
#pragma unroll 1
    for (int k = 4; k >= 0; --k) {
      const int row = kOffRows + k * 9;
      double d = 0.0;
      for (int i = k; i < 9; ++i) d += L(row + i) * L(vec + i);
      d *= L(kOffBeta + k);
      for (int i = k; i < 9; ++i) L(vec + i) -= d * L(row + i);
    }
  }

  // ---- fp_constraints: the ten cubics, a row at a time in registers ----
  {
    double e[9][4];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
      for (int m = 0; m < 4; ++m) e[k][m] = L(kOffN + m * 9 + k);
    }
    {
      double row[20];
#pragma unroll
      for (int c = 0; c < 20; ++c) row[c] = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        quad_add(q, e[3 + j], e[6 + k], 1.0); quad_add(q, e[3 + k], e[6 + j], -1.0);
        cubic_add(row, q, e[i], 1.0);
      }
#pragma unroll
      for (int c = 0; c < 20; ++c) L(kOffM + c) = row[c];
    }
    double tr[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 9; ++k) quad_add(tr, e[k], e[k], 1.0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double Lm[3][10];   // row i of E E^T - 1/2 tr I
#pragma unroll
      for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int c = 0; c < 10; ++c) Lm[j][c] = i == j ? -0.5 * tr[c] : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) quad_add(Lm[j], e[3 * i + k], e[3 * j + k], 1.0);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double row[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) row[k] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) cubic_add(row, Lm[j], e[3 * j + c], 1.0);
#pragma unroll
        for (int k = 0; k < 20; ++k) L(kOffM + (1 + 3 * i + c) * 20 + k) = row[k];
      }
    }
  }

  // ---- fp_eliminate: Gauss-Jordan on the first ten columns, row pivoting ----
  double big = 0.0;
#pragma unroll 1
  for (int e = 0; e < 200; ++e) big = fmax(big, fabs(L(kOffM + e)));
#pragma unroll 1
  for (int c = 0; c < 10; ++c) {
    int piv = c;
    for (int r = c + 1; r < 10; ++r) if (fabs(L(kOffM + r * 20 + c)) > fabs(L(kOffM + piv * 20 + c))) piv = r;
    const double p = L(kOffM + piv * 20 + c);
    if (!(fabs(p) > kFivePivotTol * big)) return;   // singular: a pure rotation
#pragma unroll 1
    for (int k = 0; k < 20; ++k) { const double v = L(kOffM + piv * 20 + k); L(kOffM + piv * 20 + k) = L(kOffM + c * 20 + k); L(kOffM + c * 20 + k) = v / p; }
#pragma unroll 1
    for (int r = 0; r < 10; ++r) {
      if (r == c) continue;
      const double f = L(kOffM + r * 20 + c);
#pragma unroll 1
      for (int k = 0; k < 20; ++k) L(kOffM + r * 20 + k) -= f * L(kOffM + c * 20 + k);
    }
  }

  // ---- fp_reduce (into rows 0..2 of the matrix's place, which nothing reads any more) and fp_eliminant ----
  {
    double B[3][3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int u = kOffM + (4 + 2 * r) * 20, l = kOffM + (5 + 2 * r) * 20;
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int c = 10 + 3 * v;
        B[r][v][0] = L(u + c + 2); B[r][v][1] = L(u + c + 1) - L(l + c + 2); B[r][v][2] = L(u + c) - L(l + c + 1); B[r][v][3] = -L(l + c); B[r][v][4] = 0.0;
      }
      B[r][2][0] = L(u + 19); B[r][2][1] = L(u + 18) - L(l + 19); B[r][2][2] = L(u + 17) - L(l + 18); B[r][2][3] = L(u + 16) - L(l + 17); B[r][2][4] = -L(l + 16);
    }
    double p[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int i = (r + 1) % 3, j = (r + 2) % 3;
      double C[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) C[a + b] += B[i][0][a] * B[j][1][b] - B[j][0][a] * B[i][1][b];
      }
#pragma unroll
      for (int a = 0; a < 7; ++a) {
#pragma unroll
        for (int b = 0; b < 5; ++b) p[a + b] += C[a] * B[r][2][b];
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int v = 0; v < 3; ++v) {
#pragma unroll
        for (int k = 0; k < 5; ++k) L(kOffB + (r * 3 + v) * 5 + k) = B[r][v][k];
      }
    }
#pragma unroll
    for (int k = 0; k < 11; ++k) L(ladder(10) + k) = p[k];
  }

  // ---- fp_roots_unit twice (p on [-1, 1]; the reversed polynomial, whose roots w are 1 / z), each root to fp_solution as it is found ----
  int count = 0;
  bool finite = true;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) {
      for (int k = 0; k < 5; ++k) { const double lo = L(ladder(10) + k); L(ladder(10) + k) = L(ladder(10) + 10 - k); L(ladder(10) + 10 - k) = lo; }
    }
#pragma unroll 1
    for (int d = 10; d >= 2; --d) for (int k = 0; k < d; ++k) L(ladder(d - 1) + k) = (k + 1) * L(ladder(d) + k + 1);
    L(kOffEdge) = -1.0; L(kOffEdge + 1) = 1.0;
#pragma unroll 1
    for (int d = 1; d <= 10; ++d) {
      double lo = -1.0;
#pragma unroll 1
      for (int i = 0; i < d; ++i) {
        const double hi = L(kOffEdge + i + 1);   // (the bracket of the level below, read before this level's root takes its place)
        double root;
        const bool found = L.bisect(ladder(d), d, lo, hi, &root);
        L(kOffEdge + i + 1) = root;
        lo = hi;
        if (d < 10 || !found) continue;
        double x = root;
        for (int it = 0; it < kFiveNewton; ++it) {
          const double xn = x - L.eval(ladder(10), 10, x) / L.eval(ladder(9), 9, x);
          if (xn >= -1.0 && xn <= 1.0) x = xn;
        }
        if (pass && (x == 1.0 || x == -1.0)) continue;   // (|z| = 1 belongs to the first pass)
        if (count == 10 || !finite) continue;
        finite = solution(L, pass ? 1.0 / x : x, count);
        if (finite) ++count;
      }
      L(kOffEdge + d + 1) = 1.0;
    }
  }
  if (!finite || count == 0) return;

  // ---- the order: ascending key, equal keys in the order found ----
#pragma unroll 1
  for (int s = 0; s < count; ++s) {
    const double ks = L(kOffKey + s);
    int rank = 0;
    for (int o = 0; o < count; ++o) { const double ko = L(kOffKey + o); if (ko < ks || (ko == ks && o < s)) ++rank; }
    for (int m = 0; m < 9; ++m) A.E_out[((size_t)t * 10 + rank) * 9 + m] = L(kOffSol + s * 9 + m);
    A.slot_status[(size_t)t * 10 + s] = 1;
  }
  A.num_solutions[t] = count;
  A.status[t] = 1;
}

__global__ __launch_bounds__(256) void epipolar_pick_kernel(const EpiPickArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.num_tasks) return;
  int best = -1, best_inl = 0, best_front = 0;
  for (int s = 0; s < 10; ++s) {
    const size_t slot = (size_t)t * 10 + s;
    if (!A.slot_status[slot]) continue;
    const int inl = A.slot_inliers[slot];
    int most = A.slot_front[slot * 4];
    for (int c = 1; c < 4; ++c) most = max(most, A.slot_front[slot * 4 + c]);
    if (best >= 0 && (inl < best_inl || (inl == best_inl && most <= best_front))) continue;
    best = s; best_inl = inl; best_front = most;
  }
  A.status[t] = best >= 0 ? 1 : 0;
  A.num_inliers[t] = best >= 0 ? best_inl : 0;
  for (int c = 0; c < 4; ++c) A.num_front[(size_t)t * 4 + c] = best >= 0 ? A.slot_front[((size_t)t * 10 + best) * 4 + c] : 0;
  if (best < 0) return;
  for (int k = 0; k < 9; ++k) A.E_out[(size_t)t * 9 + k] = A.slot_E[((size_t)t * 10 + best) * 9 + k];
  for (int k = 0; k < 6; ++k) A.poses_out[(size_t)t * 6 + k] = A.slot_poses[((size_t)t * 10 + best) * 6 + k];
}

}  // namespace

// kFiveLanes subsets per workgroup, kFiveLanes x 258 doubles of LDS: 132 096 bytes with 64 lanes, above a default launch's 64 KB and inside
// the CU's 160 KB, so the kernel's limit is raised (as pnp_dlt_kernel's is).  32 lanes per workgroup (66 048 bytes, half the wave idle)
// were measured beside it: the same time at 1 024 subsets, 4 % slower at 16 384 — the kernel is one wave's dependent chain
// either way, so the full wave stays.
hipError_t launch_epipolar_five_point(const EpiFiveArgs& A, hipStream_t st) {
  const size_t lds = (size_t)kFiveDoubles * kFiveLanes * sizeof(double);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&epipolar_five_point_kernel<kFiveLanes>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(epipolar_five_point_kernel<kFiveLanes>, dim3((A.num_tasks + kFiveLanes - 1) / kFiveLanes), dim3(kFiveLanes), lds, st, A);
  return hipGetLastError();
}
hipError_t launch_epipolar_pick(const EpiPickArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(epipolar_pick_kernel, dim3((A.num_tasks + 255) / 256), dim3(256), 0, st, A);
  return hipGetLastError();
}

}  // namespace rsba
