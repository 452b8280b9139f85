// The selected inverse of the reduced camera system: every tile of Sigma = S^-1 on the pattern of the tile Cholesky factor, from the
// factor cholesky.hip leaves (W_j = L_jj^-1 by tile index in sv.Winv, L_ij by packed slot in sv.Lf), by the Takahashi recurrence over
// the lists of chol_plan.hpp (selinv_plan):
//   G     G_kj     = L_kj W_j
//   OFF   Sigma_ij = - sum_{k in col[j]} Sigma_ik G_kj
//   DIAG  Sigma_jj = W_j^T W_j - sum_{k in col[j]} Sigma_kj^T G_kj,  stored as (X + X^T) / 2
// One 256-thread workgroup per output tile; both operands of a product are staged in LDS (a transposed operand is transposed on the way
// in), the 48 x 48 x 48 product runs on the fp64 matrix cores (v_mfma_f64_16x16x4_f64: the nine 16 x 16 blocks of the result dealt to
// the four waves, twelve steps of k each) in the register layout of chol_tasks.hpp (lane (r, g): rows g + 4v of column r).  The terms of
// a sum are taken in list order by one workgroup, so two runs agree bit for bit.  No workgroup waits for another: the host launches
// level after level, descending (solver.hip), OFF before DIAG.
//
// Decoupled coordinates.  A fixed coordinate, one no residual touches and a padding row each sit in the undamped S as a decoupled
// diagonal of 1e-6 / 1e300: W_cc ~ 1e153 with nothing else in its row and column, (W^T W)_cc ~ 1e306, and one product further is inf,
// then inf * 0 = NaN all over Sigma.  cov_live_kernel marks the coordinates that ARE unknowns — a pose coordinate that is free
// (mask_pose) and touched (udiag != 0), an intrinsics coordinate of a block in the program (inprog_intr), nothing in the padding: the rule
// of rsba_pose_covariance — and row and column c of W_j are zeroed everywhere else before G and DIAG use it.  The factor's rows and
// columns are exactly zero off the diagonal there, so Sigma gets exact zeros in these rows and columns, by induction over the recurrence.
//
// The products.  chol_tasks.hpp's accumulate() / times_inverse_transposed are written for its persistent driver: one operand comes out of
// the write-once cells with the driver's acquire loads and the other is pinned to the register image of the task before, and both
// assume the task's own LDS map.  Here every operand is a finished tile in HBM and a third of them is read transposed, so the products
// are restated (Acc: the same instruction, the same lane (r, g) -> rows g + 4 v of column r layout of the result) over two LDS tiles.
//
// cov_point_kernel: the 3 x 3 covariance block of a point from Sigma (see there).
#include "pass_common.hpp"
#include "slot_record.hpp"

namespace rsba {

namespace {

constexpr int T = kTile;
constexpr int TP = T + 1;   // LDS row pitch (doubles): odd, so that a transposed store walks the banks
typedef double dbl4_t __attribute__((ext_vector_type(4)));

// a row-major T x T tile from HBM into LDS (pitch TP), transposed on request
__device__ __forceinline__ void stage(double* dst, const double* src, bool trans, int tid) {
  for (int e = tid; e < T * T; e += 256) { const int r = e / T, c = e % T; dst[trans ? c * TP + r : r * TP + c] = src[e]; }
}
// W_j with the rows and columns of the coordinates that are no unknowns zeroed (s_live: the tile's 48 marks, in LDS)
__device__ __forceinline__ void stage_w(double* dst, const double* W, const double* s_live, bool trans, int tid) {
  for (int e = tid; e < T * T; e += 256) {
    const int r = e / T, c = e % T;
    dst[trans ? c * TP + r : r * TP + c] = (s_live[r] != 0.0 && s_live[c] != 0.0) ? W[e] : 0.0;
  }
}

// this wave's blocks of the result: b = wave, wave + 4, wave + 8 (< 9), block row b / 3, block column b % 3
struct Acc {
  dbl4_t c[3];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int n = 0; n < 3; ++n) c[n] = dbl4_t{0.0, 0.0, 0.0, 0.0};
  }
  // += sign * A B, both T x T in LDS
  __device__ __forceinline__ void mac(const double* A, const double* B, double sign, int wave, int lane) {
    const int mi = lane & 15, mg = lane >> 4;
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int b = wave + 4 * n;
      if (b < 9) {
        const int I = b / 3, J = b % 3;
#pragma unroll
        for (int kk = 0; kk < T / 4; ++kk)
          c[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(sign * A[(16 * I + mi) * TP + 4 * kk + mg], B[(4 * kk + mg) * TP + 16 * J + mi], c[n], 0, 0, 0);
      }
    }
  }
  // to a row-major tile of the given pitch (HBM: T, LDS: TP)
  __device__ __forceinline__ void store(double* out, int pitch, int wave, int lane) const {
    const int mi = lane & 15, mg = lane >> 4;
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int b = wave + 4 * n;
      if (b < 9) {
        const int I = b / 3, J = b % 3;
#pragma unroll
        for (int v = 0; v < 4; ++v) out[(16 * I + mg + 4 * v) * pitch + 16 * J + mi] = c[n][v];
      }
    }
  }
};

__global__ __launch_bounds__(256) void selinv_g_kernel(const double* Lf, const double* Winv, const double* live, const int32_t* g_info, int first, double* G) {
  __shared__ double sA[T * TP], sB[T * TP], s_live[T];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = first + blockIdx.x;
  const int slot = g_info[2 * item], tile = g_info[2 * item + 1];
  if (tid < T) s_live[tid] = live[(size_t)tile * T + tid];
  __syncthreads();
  stage(sA, Lf + (size_t)slot * (T * T), false, tid);
  stage_w(sB, Winv + (size_t)tile * (T * T), s_live, false, tid);
  __syncthreads();
  Acc acc; acc.clear();
  acc.mac(sA, sB, 1.0, wave, lane);
  acc.store(G + (size_t)slot * (T * T), T, wave, lane);
}

__global__ __launch_bounds__(256) void selinv_off_kernel(const int32_t* off_info, const int32_t* off_ptr, const int32_t* off_list, int first, double* Sigma, const double* G) {
  __shared__ double sA[T * TP], sB[T * TP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = first + blockIdx.x;
  const int out = off_info[2 * item];
  Acc acc; acc.clear();
  for (int q = off_ptr[item]; q < off_ptr[item + 1]; ++q) {
    const int ss = off_list[3 * q], trans = off_list[3 * q + 1], gs = off_list[3 * q + 2];
    __syncthreads();   // (the product before this one has read both buffers)
    stage(sA, Sigma + (size_t)ss * (T * T), trans != 0, tid);
    stage(sB, G + (size_t)gs * (T * T), false, tid);
    __syncthreads();
    acc.mac(sA, sB, -1.0, wave, lane);
  }
  acc.store(Sigma + (size_t)out * (T * T), T, wave, lane);
}

__global__ __launch_bounds__(256) void selinv_diag_kernel(const double* Winv, const double* live, const int32_t* diag_info, const int32_t* diag_ptr, const int32_t* diag_list, int first, double* Sigma,
                                                          const double* G) {
  __shared__ double sA[T * TP], sB[T * TP], s_live[T];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = first + blockIdx.x;
  const int out = diag_info[2 * item], tile = diag_info[2 * item + 1];
  const double* W = Winv + (size_t)tile * (T * T);
  if (tid < T) s_live[tid] = live[(size_t)tile * T + tid];
  __syncthreads();
  stage_w(sA, W, s_live, true, tid);
  stage_w(sB, W, s_live, false, tid);
  __syncthreads();
  Acc acc; acc.clear();
  acc.mac(sA, sB, 1.0, wave, lane);   // W^T W
  for (int q = diag_ptr[item]; q < diag_ptr[item + 1]; ++q) {
    const int s = diag_list[q];
    __syncthreads();
    stage(sA, Sigma + (size_t)s * (T * T), true, tid);   // Sigma_kj^T
    stage(sB, G + (size_t)s * (T * T), false, tid);
    __syncthreads();
    acc.mac(sA, sB, -1.0, wave, lane);
  }
  __syncthreads();
  acc.store(sA, TP, wave, lane);
  __syncthreads();
  double* o = Sigma + (size_t)out * (T * T);
  for (int e = tid; e < T * T; e += 256) { const int r = e / T, c = e % T; o[e] = 0.5 * (sA[r * TP + c] + sA[c * TP + r]); }
}

// desc [n][8]: {first row, first column (camera-side scalar indices), piece (row tile lo / hi) x (column tile lo / hi): 2 * slot + transposed, -1 = not needed}
__global__ void cov_gather_kernel(const double* Sigma, const int32_t* desc, int64_t n, int dim, double* out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * dim * dim) return;
  const int64_t p = e / (dim * dim);
  const int r = (int)(e % (dim * dim)) / dim, c = (int)(e % (dim * dim)) % dim;
  const int32_t* d = desc + 8 * p;
  const int gr = d[0] % T + r, gc = d[1] % T + c;   // (a block is shorter than a tile: at most one edge each way)
  const int piece = d[2 + 2 * (gr >= T) + (gc >= T)];
  double v = 0.0;
  if (piece >= 0) {
    const int lr = gr % T, lc = gc % T;
    const double* tile = Sigma + (size_t)(piece >> 1) * (T * T);
    v = (piece & 1) ? tile[lc * T + lr] : tile[lr * T + lc];
  }
  out[e] = v;
}

// live[i] = 1 where camera-side coordinate i is an unknown of the program, 0 elsewhere (see the head of this file)
__global__ void cov_live_kernel(const SolverDev sv, const double* mask_pose, double* live) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sv.npad) return;
  const int64_t n = (int64_t)sv.F * sv.CD, nx = (int64_t)sv.Fx * sv.CD;
  double v = 0.0;
  if (i < n) v = (mask_pose[i] != 0.0 && sv.udiag[i] != 0.0) ? 1.0 : 0.0;
  else if (i < nx && sv.inprog_intr) v = sv.inprog_intr[i - n] != 0.0 ? 1.0 : 0.0;
  live[i] = v;
}

// entry (r, c) of Sigma by camera-side scalar indices; tmap [nt][nt]: 2 * slot + transposed of the tile pair, -1 = not on the pattern
__device__ __forceinline__ double sigma_at(const double* Sigma, const int32_t* tmap, int nt, int r, int c, int* missing) {
  const int piece = tmap[(size_t)(r / T) * nt + c / T];
  if (piece < 0) { atomicOr(missing, 1); return 0.0; }
  const double* tile = Sigma + (size_t)(piece >> 1) * (T * T);
  const int lr = r % T, lc = c % T;
  return (piece & 1) ? tile[lc * T + lr] : tile[lr * T + lc];
}

// Covariance block of point j = points[blockIdx.x]:
//   Cov_j = V^-1 + V^-1 ( sum_o sum_o' W_o^T Sigma_{c(o) c(o')} W_o' ) V^-1 + q q^T * border_scale,   q = V^-1 sum_o W_o^T v_{c(o)}
// with W_o = X_o^T Jp_o, X_o = [Ji_o | Jc_o] the 2 x (9 +) CD camera-side Jacobian of observation o — recomputed from the observation
// as every point-side pass does (lm_record.hpp: loss-corrected, zero in fixed columns) — c(o) its coordinates (the frame's intrinsics
// block at the front of its pseudo frames, then the frame's poses), V^-1 = Linv^T Linv from the point factor of the undamped system.
// Written as sum_o sum_o' Jp_o^T (X_o Sigma X_o'^T) Jp_o': a 2 x 2 matrix per pair.  One wave per point: lane l takes o = l, l + 64, ...
// against every o' in slot order, the lanes' 3 x 3 sums are added in lane order by lane 0 — fixed order, two calls agree bit for bit.
struct CovPointArgs {
  const double* Sigma; const int32_t* tmap; const double* v; double border_scale;
  const int32_t* points; const double2* slot_xy; double* out; int* missing;
};
// the record of slot s (slot_record.hpp: the point-side passes' own) and rows[]: where its camera-side columns sit in Sigma
template <bool CAL, int P, bool GEN>
__device__ __forceinline__ void cov_slot_record(const DeviceProblem& dp, const SolverDev& sv, const double2* slot_xy, int64_t s, ObsOut<CAL, P>& o, int rows[(CAL ? 0 : 9) + 6 * P]) {
  constexpr int CD = 6 * P, OP = CAL ? 0 : 9;
  int frame, point;
  slot_record<CAL, P, GEN>(dp, sv, slot_xy, s, o, frame, point);
  if (!CAL) {
    const int r0 = (sv.F + (sv.NIB > 1 ? dp.frame_intr[frame] : 0) * sv.NPF) * CD;
#pragma unroll
    for (int k = 0; k < 9; ++k) rows[k] = r0 + k;
  }
#pragma unroll
  for (int k = 0; k < CD; ++k) rows[OP + k] = frame * CD + k;
}
template <bool CAL, int P, bool GEN>
__global__ __launch_bounds__(64) void cov_point_kernel(const DeviceProblem dp, const SolverDev sv, const CovPointArgs a) {
  constexpr int CD = 6 * P, OP = CAL ? 0 : 9, K = OP + CD;
  __shared__ double red[64 * 12];
  const int lane = threadIdx.x;
  const int64_t j = a.points ? a.points[blockIdx.x] : (int64_t)blockIdx.x;
  const int64_t lo = sv.point_ptr[j], hi = sv.point_ptr[j + 1];
  double acc[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) acc[q] = 0.0;
  for (int64_t s = lo + lane; s < hi; s += 64) {
    ObsOut<CAL, P> o; int rows[K];
    cov_slot_record<CAL, P, GEN>(dp, sv, a.slot_xy, s, o, rows);
    if (a.v) {   // the border's column: Jp_o^T (X_o v)
      double b0 = 0.0, b1 = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) { const double vv = a.v[rows[k]]; b0 += o.J[0][k] * vv; b1 += o.J[1][k] * vv; }
#pragma unroll
      for (int x = 0; x < 3; ++x) acc[9 + x] += o.J[0][K + x] * b0 + o.J[1][K + x] * b1;
    }
    for (int64_t s2 = lo; s2 < hi; ++s2) {
      ObsOut<CAL, P> o2; int rows2[K];
      cov_slot_record<CAL, P, GEN>(dp, sv, a.slot_xy, s2, o2, rows2);
      double m00 = 0.0, m01 = 0.0, m10 = 0.0, m11 = 0.0;   // X_o Sigma X_o2^T
#pragma unroll
      for (int k = 0; k < K; ++k) {
        double w0 = 0.0, w1 = 0.0;
#pragma unroll
        for (int k2 = 0; k2 < K; ++k2) { const double sg = sigma_at(a.Sigma, a.tmap, sv.nt, rows[k], rows2[k2], a.missing); w0 += sg * o2.J[0][k2]; w1 += sg * o2.J[1][k2]; }
        m00 += o.J[0][k] * w0; m01 += o.J[0][k] * w1; m10 += o.J[1][k] * w0; m11 += o.J[1][k] * w1;
      }
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const double l0 = o.J[0][K + x] * m00 + o.J[1][K + x] * m10, l1 = o.J[0][K + x] * m01 + o.J[1][K + x] * m11;
#pragma unroll
        for (int y = 0; y < 3; ++y) acc[3 * x + y] += l0 * o2.J[0][K + y] + l1 * o2.J[1][K + y];
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 12; ++q) red[lane * 12 + q] = acc[q];
  __syncthreads();
  if (lane != 0) return;
  double m[12];
  for (int q = 0; q < 12; ++q) { double t = 0.0; for (int l = 0; l < 64; ++l) t += red[l * 12 + q]; m[q] = t; }
  const double* li = sv.Linv + (size_t)j * 6;
  const double L[3][3] = {{li[0], 0.0, 0.0}, {li[1], li[2], 0.0}, {li[3], li[4], li[5]}};
  double vi[3][3], t1[3][3], c[3][3], q3[3];
  for (int x = 0; x < 3; ++x) for (int y = 0; y < 3; ++y) vi[x][y] = L[0][x] * L[0][y] + L[1][x] * L[1][y] + L[2][x] * L[2][y];
  for (int x = 0; x < 3; ++x) for (int y = 0; y < 3; ++y) t1[x][y] = vi[x][0] * m[y] + vi[x][1] * m[3 + y] + vi[x][2] * m[6 + y];
  for (int x = 0; x < 3; ++x) q3[x] = vi[x][0] * m[9] + vi[x][1] * m[10] + vi[x][2] * m[11];
  for (int x = 0; x < 3; ++x) for (int y = 0; y < 3; ++y)
    c[x][y] = vi[x][y] + (t1[x][0] * vi[0][y] + t1[x][1] * vi[1][y] + t1[x][2] * vi[2][y]) + q3[x] * q3[y] * a.border_scale;
  double* out = a.out + (size_t)blockIdx.x * 9;
  const bool none = lo == hi;   // (a point nobody sees is no unknown of the program)
  for (int x = 0; x < 3; ++x) for (int y = 0; y < 3; ++y) out[3 * x + y] = none ? 0.0 : 0.5 * (c[x][y] + c[y][x]);
}

}  // namespace

hipError_t launch_selinv_g(const SolverDev& sv, const SelinvPlan& pl, const double* live, double* G, int first, int count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(selinv_g_kernel, dim3(count), dim3(256), 0, st, sv.Lf, sv.Winv, live, pl.g_info, first, G);
  return hipGetLastError();
}
hipError_t launch_selinv_off(const SelinvPlan& pl, double* Sigma, const double* G, int first, int count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(selinv_off_kernel, dim3(count), dim3(256), 0, st, pl.off_info, pl.off_ptr, pl.off_list, first, Sigma, G);
  return hipGetLastError();
}
hipError_t launch_selinv_diag(const SolverDev& sv, const SelinvPlan& pl, const double* live, double* Sigma, const double* G, int first, int count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(selinv_diag_kernel, dim3(count), dim3(256), 0, st, sv.Winv, live, pl.diag_info, pl.diag_ptr, pl.diag_list, first, Sigma, G);
  return hipGetLastError();
}
hipError_t launch_cov_gather(const double* Sigma, const int32_t* desc, int64_t n, int dim, double* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t total = n * dim * dim;
  hipLaunchKernelGGL(cov_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Sigma, desc, n, dim, out);
  return hipGetLastError();
}

hipError_t launch_cov_live(const SolverDev& sv, const double* mask_pose, double* live, hipStream_t st) {
  hipLaunchKernelGGL(cov_live_kernel, dim3((unsigned)((sv.npad + 255) / 256)), dim3(256), 0, st, sv, mask_pose, live);
  return hipGetLastError();
}
hipError_t launch_cov_points(const DeviceProblem& dp, const SolverDev& sv, const double* Sigma, const int32_t* tmap, const double* v, double border_scale, const int32_t* points,
                             int64_t n, const double2* slot_xy, double* out, int* missing, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const CovPointArgs a{Sigma, tmap, v, border_scale, points, slot_xy, out, missing};
  with_record_variant(dp, sv, [&](auto cal, auto two, auto gen) {
    hipLaunchKernelGGL((cov_point_kernel<decltype(cal)::value, decltype(two)::value ? 2 : 1, decltype(gen)::value>), dim3((unsigned)n), dim3(64), 0, st, dp, sv, a);
  });
  return hipGetLastError();
}

}  // namespace rsba
