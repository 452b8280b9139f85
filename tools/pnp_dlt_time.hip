// Times the DLT start poses of RANSAC hypotheses (tools/pnp_dlt_time.py builds and runs this): for 500, 1 000 and 16 384 six-point
// subsets of 2 000 points, the wall time of the host loop over pnp_detail::dlt_pose (include/rsba/solve_rs_pnp.hpp) and the HIP-event
// time of the device kernels (normalise + DLT, kernels_pnp_dlt.hip, included here so that the events bracket the launches alone: no
// allocation, no copy).  One JSON line per size.  Also checks that both give the same statuses and poses.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../rsba_amd/csrc/kernels_pnp_dlt.hip"
#include "pnp_time_scene.hpp"
#include "rsba/solve_rs_pnp.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  const int n = 2000, m = 6;
  const PnpTimeScene sc(n);
  rsba::PnpDltArgs A{};
  for (int k = 0; k < 9; ++k) A.cam[k] = sc.cam[k];
  float *d_op, *d_ip; double* d_nrm;
  CHECK(hipMalloc(&d_op, sizeof(float) * 3 * n)); CHECK(hipMalloc(&d_ip, sizeof(float) * 2 * n)); CHECK(hipMalloc(&d_nrm, sizeof(double) * 2 * n));
  CHECK(hipMemcpy(d_op, sc.X.data(), sizeof(float) * 3 * n, hipMemcpyHostToDevice)); CHECK(hipMemcpy(d_ip, sc.xy.data(), sizeof(float) * 2 * n, hipMemcpyHostToDevice));
  A.n = n; A.m = m; A.object_points = d_op; A.image_points = d_ip; A.normalised = d_nrm;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  for (int T : {500, 1000, 16384}) {
    const std::vector<int32_t> subs = sc.subsets(T, m);
    // host: normalise once, dlt_pose per subset; best of 5
    std::vector<double> hp((size_t)T * 6, 0.0); std::vector<uint8_t> hs((size_t)T);
    double host_ms = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
      const auto t0 = std::chrono::steady_clock::now();
      const std::vector<double> nrm = rsba_amd::hyp_detail::normalised_points(sc.cam, sc.xy.data(), n);
      for (int t = 0; t < T; ++t) hs[(size_t)t] = rsba_amd::pnp_detail::dlt_pose(sc.X.data(), nrm.data(), &subs[(size_t)t * m], m, &hp[(size_t)t * 6]);
      host_ms = std::fmin(host_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    int32_t* d_sub; double* d_poses; uint8_t* d_st;
    CHECK(hipMalloc(&d_sub, sizeof(int32_t) * subs.size())); CHECK(hipMalloc(&d_poses, sizeof(double) * 6 * T)); CHECK(hipMalloc(&d_st, T));
    CHECK(hipMemcpy(d_sub, subs.data(), sizeof(int32_t) * subs.size(), hipMemcpyHostToDevice));
    A.num_tasks = T; A.subsets = d_sub; A.poses_out = d_poses; A.status = d_st;
    for (int w = 0; w < 3; ++w) { CHECK(rsba::launch_pnp_normalise(A, nullptr)); CHECK(rsba::launch_pnp_dlt(A, nullptr)); }
    CHECK(hipDeviceSynchronize());
    double dev_ms = 1e30, dev_sum = 0.0; const int reps = 20;
    for (int rep = 0; rep < reps; ++rep) {
      CHECK(hipEventRecord(e0, nullptr));
      CHECK(rsba::launch_pnp_normalise(A, nullptr)); CHECK(rsba::launch_pnp_dlt(A, nullptr));
      CHECK(hipEventRecord(e1, nullptr)); CHECK(hipEventSynchronize(e1));
      float ms = 0; CHECK(hipEventElapsedTime(&ms, e0, e1));
      dev_ms = std::fmin(dev_ms, (double)ms); dev_sum += ms;
    }
    std::vector<double> dp((size_t)T * 6); std::vector<uint8_t> ds((size_t)T);
    CHECK(hipMemcpy(dp.data(), d_poses, sizeof(double) * 6 * T, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(ds.data(), d_st, T, hipMemcpyDeviceToHost));
    int status_mismatch = 0, accepted = 0; double worst = 0.0;
    for (int t = 0; t < T; ++t) {
      status_mismatch += (ds[(size_t)t] != 0) != (hs[(size_t)t] != 0);
      if (ds[(size_t)t] && hs[(size_t)t]) { ++accepted; for (int k = 0; k < 6; ++k) worst = std::fmax(worst, std::fabs(dp[(size_t)t * 6 + k] - hp[(size_t)t * 6 + k])); }
    }
    std::printf("{\"subsets\": %d, \"points\": %d, \"host_dlt_loop_ms\": %.4f, \"device_dlt_event_ms_min\": %.4f, \"device_dlt_event_ms_mean\": %.4f, "
                "\"accepted\": %d, \"status_mismatches\": %d, \"worst_pose_difference\": %.3g}\n", T, n, host_ms, dev_ms, dev_sum / reps, accepted, status_mismatch, worst);
    CHECK(hipFree(d_sub)); CHECK(hipFree(d_poses)); CHECK(hipFree(d_st));
  }
  return 0;
}
