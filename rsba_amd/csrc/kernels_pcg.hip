// Block-Jacobi preconditioned conjugate gradients on the explicit reduced camera system (the rule: include/rsba_amd.h,
// rsba_set_linear_solver; the lists: pcg.hpp / pcg_plan.cpp).
//
// Three launches per iteration, none of which waits for another workgroup:
//   product   one workgroup per row tile of S: p = z + beta p_old formed as it is read, q = S p over the row's tiles in list order
//             (each tile through LDS; lower tiles serve their row as stored and their column transposed), partial p.q
//   update    one thread per block of the preconditioner: alpha = r.z / p.q, y += alpha p, r -= alpha q, z = M^-1 r through the
//             block's Cholesky factor, partial r.z, r.r, y.(rhs + r) per workgroup
//   decide    one workgroup: the sums, Q_k, the stopping tests, beta; sets the flag every kernel reads first
// Every sum has one order: a thread's own terms in index order, lanes by a fixed xor tree, workgroups by fixed_sum below.  The
// result does not depend on which workgroup ran when, nor on the numbering of the packed slots.
#include "solver_state.hpp"
#include "pcg.hpp"

namespace rsba {

namespace {

constexpr int T = kTile, TP = kTile + 1;
constexpr int kTri = kPcgBlockMax * (kPcgBlockMax + 1) / 2;

// sum of v[0 .. n) by the `width` threads of a workgroup whose threads all call it: thread t adds v[t], v[t + width], ... in that
// order, then the partial sums meet in a fixed tree; every thread returns the same bits, and so does every workgroup of the same width.
template <int WIDTH>
__device__ __forceinline__ double fixed_sum(const double* __restrict__ v, int n, double* lds) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += WIDTH) s += v[i];
  __syncthreads();   // (lds may still be read from the call before)
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int w = WIDTH / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
    __syncthreads();
  }
  return lds[0];
}

__device__ __forceinline__ double direction(double z, double beta, double p_old) { return fma(beta, p_old, z); }

// z = M_b^-1 r for one block: L w = r, L^T z = w with the packed factor of block b (diagonal stored inverted)
__device__ __forceinline__ void block_solve(const double* __restrict__ fac, int nblk, int b, int m, const double* r, double* z) {
  double w[kPcgBlockMax];
  for (int i = 0; i < m; ++i) {
    double s = r[i];
    for (int k = 0; k < i; ++k) s -= fac[(size_t)(i * (i + 1) / 2 + k) * nblk + b] * w[k];
    w[i] = s * fac[(size_t)(i * (i + 1) / 2 + i) * nblk + b];
  }
  for (int i = m - 1; i >= 0; --i) {
    double s = w[i];
    for (int k = i + 1; k < m; ++k) s -= fac[(size_t)(k * (k + 1) / 2 + i) * nblk + b] * z[k];
    z[i] = s * fac[(size_t)(i * (i + 1) / 2 + i) * nblk + b];
  }
}

// the three sums of a workgroup of the per-block kernels (one wave): fixed xor tree, lane 0 stores
__device__ __forceinline__ void store_partials(const PcgDev& pc, double a, double b, double c) {
  for (int w = 32; w > 0; w >>= 1) { a += __shfl_xor(a, w, 64); b += __shfl_xor(b, w, 64); c += __shfl_xor(c, w, 64); }
  if (threadIdx.x == 0) { pc.part[blockIdx.x] = a; pc.part[pc.nbw + blockIdx.x] = b; pc.part[2 * pc.nbw + blockIdx.x] = c; }
}

// Factors of the blocks of M = blockdiag(S), then the state of iteration 0: y = 0, r = rhs, z = M^-1 r, p_old = 0.
__global__ __launch_bounds__(kPcgBlockThreads) void pcg_begin_kernel(const SolverDev sv, const PcgDev pc) {
  const int b = blockIdx.x * kPcgBlockThreads + threadIdx.x;
  double rz = 0.0, rr = 0.0;
  if (b < pc.nblk) {
    const int row0 = pc.blk_row[b], m = pc.blk_size[b], t0 = row0 / T;
    const int s0 = pc.blk_slots[3 * b], s1 = pc.blk_slots[3 * b + 1], s2 = pc.blk_slots[3 * b + 2];
    double A[kTri];
    for (int i = 0; i < m; ++i)
      for (int j = 0; j <= i; ++j) {
        const int gr = row0 + i, gc = row0 + j, ti = gr / T, tj = gc / T, r = gr % T, c = gc % T;
        double v = 0.0;
        if (ti == tj) v = sv.S[(size_t)(ti == t0 ? s0 : s1) * (T * T) + r * T + c];   // (a diagonal tile is read through its lower triangle: r >= c here)
        else if (s2 >= 0) v = sv.S[(size_t)(s2 >> 1) * (T * T) + ((s2 & 1) ? c * T + r : r * T + c)];
        A[i * (i + 1) / 2 + j] = v;
      }
    bool bad = false;
    for (int j = 0; j < m; ++j) {
      double d = A[j * (j + 1) / 2 + j];
      for (int k = 0; k < j; ++k) d -= A[j * (j + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
      if (!(d > 0.0) || !isfinite(d)) { bad = true; d = 1.0; }
      const double inv = 1.0 / sqrt(d);
      A[j * (j + 1) / 2 + j] = inv;
      for (int i = j + 1; i < m; ++i) {
        double s = A[i * (i + 1) / 2 + j];
        for (int k = 0; k < j; ++k) s -= A[i * (i + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
        A[i * (i + 1) / 2 + j] = s * inv;
      }
    }
    if (bad) atomicExch(sv.chol_fail, 1);
    for (int e = 0; e < m * (m + 1) / 2; ++e) pc.fac[(size_t)e * pc.nblk + b] = A[e];
    double rv[kPcgBlockMax], zv[kPcgBlockMax];
    for (int i = 0; i < m; ++i) rv[i] = sv.rhs[row0 + i];
    block_solve(pc.fac, pc.nblk, b, m, rv, zv);
    for (int i = 0; i < m; ++i) {
      pc.y[row0 + i] = 0.0; pc.r[row0 + i] = rv[i]; pc.z[row0 + i] = zv[i]; pc.p[0][row0 + i] = 0.0;
      rz += rv[i] * zv[i]; rr += rv[i] * rv[i];
    }
  }
  store_partials(pc, rz, rr, 0.0);
}

__global__ __launch_bounds__(256) void pcg_begin_scalars_kernel(const SolverDev sv, const PcgDev pc) {
  __shared__ double lds[256];
  const double rz = fixed_sum<256>(pc.part, pc.nbw, lds);
  const double b2 = fixed_sum<256>(pc.part + pc.nbw, pc.nbw, lds);
  if (threadIdx.x == 0) {
    double* sc = pc.sc;
    sc[kPcgK] = 0.0; sc[kPcgRz] = rz; sc[kPcgBeta] = 0.0; sc[kPcgQ] = 0.0; sc[kPcgB2] = b2; sc[kPcgRel] = b2 > 0.0 ? 1.0 : 0.0; sc[kPcgZeta] = 0.0;
    // a failed block (or a failed point block before it: the step is invalid either way) ends the solve before it starts; rhs = 0 is solved by y = 0
    sc[kPcgDone] = (*sv.chol_fail != 0 || !isfinite(rz) || !isfinite(b2)) ? 3.0 : (b2 == 0.0 ? 1.0 : 0.0);
    if (!isfinite(rz) || !isfinite(b2)) *sv.chol_fail = 1;
  }
}

// q = S p for the rows of one tile, p = z + beta p_old
__global__ __launch_bounds__(4 * kTile) void pcg_product_kernel(const SolverDev sv, const PcgDev pc, int flip) {
  if (pc.sc[kPcgDone] != 0.0) return;
  __shared__ double tile[T * TP];
  __shared__ double pj[T], red[T];
  const int I = blockIdx.x, tid = threadIdx.x, r = tid >> 2, l = tid & 3;
  const double beta = pc.sc[kPcgBeta];
  const double* __restrict__ p_old = pc.p[flip];
  double acc = 0.0;
  for (int e = pc.row_ptr[I]; e < pc.row_ptr[I + 1]; ++e) {
    const int slot = pc.row_list[2 * e], code = pc.row_list[2 * e + 1], J = code >> 1;
    const bool trans = (code & 1) != 0;
    __syncthreads();   // the tile before has been read
    const double* __restrict__ St = sv.S + (size_t)slot * (T * T);
    for (int x = tid; x < T * T; x += 4 * T) tile[(x / T) * TP + x % T] = St[x];
    if (tid < T) pj[tid] = direction(pc.z[(size_t)J * T + tid], beta, p_old[(size_t)J * T + tid]);
    __syncthreads();
    double s = 0.0;
    if (J == I) { for (int c = 12 * l; c < 12 * l + 12; ++c) s += tile[max(r, c) * TP + min(r, c)] * pj[c]; }
    else if (trans) { for (int c = 12 * l; c < 12 * l + 12; ++c) s += tile[c * TP + r] * pj[c]; }
    else { for (int c = 12 * l; c < 12 * l + 12; ++c) s += tile[r * TP + c] * pj[c]; }
    s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
    acc += s;
  }
  if (l == 0) {
    const double p = direction(pc.z[(size_t)I * T + r], beta, p_old[(size_t)I * T + r]);
    pc.p[flip ^ 1][(size_t)I * T + r] = p;
    pc.q[(size_t)I * T + r] = acc;
    red[r] = p * acc;
  }
  __syncthreads();
  if (tid == 0) { double s = 0.0; for (int k = 0; k < T; ++k) s += red[k]; pc.part_pq[I] = s; }
}

__global__ __launch_bounds__(kPcgBlockThreads) void pcg_update_kernel(const SolverDev sv, const PcgDev pc, int flip) {
  if (pc.sc[kPcgDone] != 0.0) return;
  __shared__ double lds[kPcgBlockThreads];
  const double pq = fixed_sum<kPcgBlockThreads>(pc.part_pq, sv.nt, lds);
  if (!(pq > 0.0) || !isfinite(pq)) return;   // (the deciding kernel fails the solve; y stays the last iterate)
  const double alpha = pc.sc[kPcgRz] / pq;
  const double* __restrict__ p = pc.p[flip ^ 1];
  const int b = blockIdx.x * kPcgBlockThreads + threadIdx.x;
  double rz = 0.0, rr = 0.0, yb = 0.0;
  if (b < pc.nblk) {
    const int row0 = pc.blk_row[b], m = pc.blk_size[b];
    double rv[kPcgBlockMax], zv[kPcgBlockMax], yv[kPcgBlockMax];
    for (int i = 0; i < m; ++i) {
      yv[i] = fma(alpha, p[row0 + i], pc.y[row0 + i]);
      rv[i] = fma(-alpha, pc.q[row0 + i], pc.r[row0 + i]);
    }
    block_solve(pc.fac, pc.nblk, b, m, rv, zv);
    for (int i = 0; i < m; ++i) {
      pc.y[row0 + i] = yv[i]; pc.r[row0 + i] = rv[i]; pc.z[row0 + i] = zv[i];
      rz += rv[i] * zv[i]; rr += rv[i] * rv[i]; yb += yv[i] * (sv.rhs[row0 + i] + rv[i]);
    }
  }
  store_partials(pc, rz, rr, yb);
}

__global__ __launch_bounds__(256) void pcg_decide_kernel(const SolverDev sv, const PcgDev pc, const PcgRule rule) {
  if (pc.sc[kPcgDone] != 0.0) return;
  __shared__ double lds[256];
  const double pq = fixed_sum<256>(pc.part_pq, sv.nt, lds);
  const bool pq_ok = pq > 0.0 && isfinite(pq);
  const double rzn = pq_ok ? fixed_sum<256>(pc.part, pc.nbw, lds) : 0.0;
  const double rr = pq_ok ? fixed_sum<256>(pc.part + pc.nbw, pc.nbw, lds) : 0.0;
  const double yb = pq_ok ? fixed_sum<256>(pc.part + 2 * pc.nbw, pc.nbw, lds) : 0.0;
  if (threadIdx.x != 0) return;
  double* sc = pc.sc;
  if (!pq_ok || !isfinite(rzn) || !isfinite(rr) || !isfinite(yb)) { *sv.chol_fail = 1; sc[kPcgDone] = 3.0; return; }
  const double k = sc[kPcgK] + 1.0, Q = -0.5 * yb, Qp = sc[kPcgQ], b2 = sc[kPcgB2];
  const double zeta = k * (Q - Qp) / Q;
  double done = 0.0;
  if (rr == 0.0) done = 1.0;   // solved exactly: there is no next direction
  if (k >= (double)rule.min_iterations) {
    if (rule.r_tolerance >= 0.0 && sqrt(rr) <= rule.r_tolerance * sqrt(b2)) done = 1.0;
    if (rule.eta > 0.0 && zeta < rule.eta) done = 1.0;
  }
  if (done == 0.0 && k >= (double)rule.max_iterations) done = 2.0;
  sc[kPcgK] = k; sc[kPcgBeta] = rzn / sc[kPcgRz]; sc[kPcgRz] = rzn; sc[kPcgQ] = Q; sc[kPcgRel] = sqrt(rr / b2); sc[kPcgZeta] = zeta;
  sc[kPcgDone] = done;
}

}  // namespace

hipError_t launch_pcg_begin(const SolverDev& sv, const PcgDev& pc, hipStream_t st) {
  hipLaunchKernelGGL(pcg_begin_kernel, dim3(pc.nbw), dim3(kPcgBlockThreads), 0, st, sv, pc);
  hipLaunchKernelGGL(pcg_begin_scalars_kernel, dim3(1), dim3(256), 0, st, sv, pc);
  return hipGetLastError();
}

hipError_t launch_pcg_iteration(const SolverDev& sv, const PcgDev& pc, const PcgRule& rule, int flip, hipStream_t st) {
  hipLaunchKernelGGL(pcg_product_kernel, dim3(sv.nt), dim3(4 * kTile), 0, st, sv, pc, flip);
  hipLaunchKernelGGL(pcg_update_kernel, dim3(pc.nbw), dim3(kPcgBlockThreads), 0, st, sv, pc, flip);
  hipLaunchKernelGGL(pcg_decide_kernel, dim3(1), dim3(256), 0, st, sv, pc, rule);
  return hipGetLastError();
}

}  // namespace rsba
