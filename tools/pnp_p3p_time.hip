// Times the minimal-solver hypotheses of the global-shutter RANSAC (tools/pnp_p3p_time.py builds and runs this) on the scene of
// pnp_time_scene.hpp, for 500, 1 000 and 16 384 subsets of 2 000 points, HIP-event time after a warm-up:
//   * the P3P kernel alone (kernels_pnp_p3p.hip, included here so that the events bracket the launch alone; the image points are
//     normalised once before),
//   * the whole rsba_pnp_gs_hypotheses_p3p call (upload, normalise, P3P, compact, refinement and scoring with m = 4, download),
//   * beside it the whole rsba_pnp_gs_hypotheses call (the DLT form, m = 6) at the same counts, in the same run.
// One JSON line per size.  Also counts the subsets the kernel and the host pnp_detail::p3p_pose disagree on.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../rsba_amd/csrc/kernels_pnp_dlt.hip"
#include "../rsba_amd/csrc/kernels_pnp_p3p.hip"
#include "pnp_time_scene.hpp"
#include "rsba/solve_rs_pnp.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define CALL(x) do { int32_t r_ = (x); if (r_ != 0) { std::fprintf(stderr, "%s: %s\n", #x, rsba_last_error()); return 1; } } while (0)

int main() {
  const int n = 2000;
  const PnpTimeScene sc(n);
  rsba::PnpDltArgs D{};
  for (int k = 0; k < 9; ++k) D.cam[k] = sc.cam[k];
  float *d_op, *d_ip; double* d_nrm;
  CHECK(hipMalloc(&d_op, sizeof(float) * 3 * n)); CHECK(hipMalloc(&d_ip, sizeof(float) * 2 * n)); CHECK(hipMalloc(&d_nrm, sizeof(double) * 2 * n));
  CHECK(hipMemcpy(d_op, sc.X.data(), sizeof(float) * 3 * n, hipMemcpyHostToDevice)); CHECK(hipMemcpy(d_ip, sc.xy.data(), sizeof(float) * 2 * n, hipMemcpyHostToDevice));
  D.n = n; D.object_points = d_op; D.image_points = d_ip; D.normalised = d_nrm;
  CHECK(rsba::launch_pnp_normalise(D, nullptr));
  const std::vector<double> nrm = rsba_amd::hyp_detail::normalised_points(sc.cam, sc.xy.data(), n);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  const int reps = 20;
  for (int T : {500, 1000, 16384}) {
    const std::vector<int32_t> sub4 = sc.subsets(T, 4), sub6 = sc.subsets(T, 6);
    int32_t* d_sub; double* d_poses; uint8_t* d_st; int32_t* d_ns;
    CHECK(hipMalloc(&d_sub, sizeof(int32_t) * sub4.size())); CHECK(hipMalloc(&d_poses, sizeof(double) * 6 * T)); CHECK(hipMalloc(&d_st, T)); CHECK(hipMalloc(&d_ns, sizeof(int32_t) * T));
    CHECK(hipMemcpy(d_sub, sub4.data(), sizeof(int32_t) * sub4.size(), hipMemcpyHostToDevice));
    rsba::PnpP3pArgs P{};
    P.n = n; P.num_tasks = T; P.object_points = d_op; P.normalised = d_nrm; P.subsets = d_sub; P.poses_out = d_poses; P.status = d_st; P.num_solutions = d_ns;
    for (int w = 0; w < 3; ++w) CHECK(rsba::launch_pnp_p3p(P, nullptr));
    CHECK(hipDeviceSynchronize());
    double k_min = 1e30, k_sum = 0.0;
    for (int rep = 0; rep < reps; ++rep) {
      CHECK(hipEventRecord(e0, nullptr));
      CHECK(rsba::launch_pnp_p3p(P, nullptr));
      CHECK(hipEventRecord(e1, nullptr)); CHECK(hipEventSynchronize(e1));
      float ms = 0; CHECK(hipEventElapsedTime(&ms, e0, e1));
      k_min = std::fmin(k_min, (double)ms); k_sum += ms;
    }
    std::vector<double> dp((size_t)T * 6); std::vector<uint8_t> ds((size_t)T);
    CHECK(hipMemcpy(dp.data(), d_poses, sizeof(double) * 6 * T, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(ds.data(), d_st, T, hipMemcpyDeviceToHost));
    int mismatch = 0, accepted = 0; double worst = 0.0;
    for (int t = 0; t < T; ++t) {
      double hp[6];
      const bool ok = rsba_amd::pnp_detail::p3p_pose(sc.X.data(), nrm.data(), &sub4[(size_t)t * 4], hp);
      mismatch += ok != (ds[(size_t)t] != 0);
      if (ok && ds[(size_t)t]) { ++accepted; for (int k = 0; k < 6; ++k) worst = std::fmax(worst, std::fabs(dp[(size_t)t * 6 + k] - hp[k])); }
    }
    // the two whole calls, alternating
    std::vector<double> poses((size_t)T * 6); std::vector<uint8_t> st((size_t)T); std::vector<int32_t> inl((size_t)T);
    double c_min[2] = {1e30, 1e30}, c_sum[2] = {0, 0}; int best[2] = {0, 0};
    for (int rep = -2; rep < reps; ++rep)
      for (int which = 0; which < 2; ++which) {
        CHECK(hipEventRecord(e0, nullptr));
        if (which == 0) CALL(rsba_pnp_gs_hypotheses_p3p(0, sc.cam, sc.X.data(), sc.xy.data(), n, sub4.data(), T, 5, 6.0f, poses.data(), st.data(), nullptr, inl.data()));
        else CALL(rsba_pnp_gs_hypotheses(0, sc.cam, sc.X.data(), sc.xy.data(), n, sub6.data(), 6, T, 5, 6.0f, poses.data(), st.data(), nullptr, inl.data()));
        CHECK(hipEventRecord(e1, nullptr)); CHECK(hipEventSynchronize(e1));
        float ms = 0; CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep >= 0) { c_min[which] = std::fmin(c_min[which], (double)ms); c_sum[which] += ms; }
        best[which] = 0;
        for (int t = 0; t < T; ++t) if (st[(size_t)t] && inl[(size_t)t] > best[which]) best[which] = inl[(size_t)t];
      }
    std::printf("{\"subsets\": %d, \"points\": %d, \"p3p_kernel_event_ms_min\": %.4f, \"p3p_kernel_event_ms_mean\": %.4f, "
                "\"gs_hypotheses_p3p_event_ms_min\": %.4f, \"gs_hypotheses_p3p_event_ms_mean\": %.4f, \"gs_hypotheses_dlt_event_ms_min\": %.4f, \"gs_hypotheses_dlt_event_ms_mean\": %.4f, "
                "\"p3p_accepted\": %d, \"status_mismatches_with_host\": %d, \"worst_pose_difference_with_host\": %.3g, \"best_inliers_p3p\": %d, \"best_inliers_dlt\": %d}\n",
                T, n, k_min, k_sum / reps, c_min[0], c_sum[0] / reps, c_min[1], c_sum[1] / reps, accepted, mismatch, worst, best[0], best[1]);
    CHECK(hipFree(d_sub)); CHECK(hipFree(d_poses)); CHECK(hipFree(d_st)); CHECK(hipFree(d_ns));
  }
  return 0;
}
