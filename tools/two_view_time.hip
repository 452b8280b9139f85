// Times the essential-matrix hypotheses of the two-view bootstrap (tools/two_view_time.py builds and runs this) on a synthetic pair of views
// (n points 6 - 12 units in front of camera A, camera B one unit to the side and slightly turned, pinhole, +-0.5 px of uniform noise), for
// T in {1024, 16384} eight-point subsets of n in {500, 8000} correspondences.  Three warm-ups, ten timed repetitions, median with min .. max:
//   * the two kernels alone, HIP events around each launch (kernels_epipolar.hip is included here so that the events bracket the launch
//     alone; both sides are normalised once before),
//   * the whole rsba_epipolar_hypotheses call (upload, normalise, eight-point, score, download), wall clock around the synchronous call,
//   * beside it the same batch from the host definitions (epi_detail::eight_point + score, one thread), once.
// One JSON line per workload.  Also counts the subsets the device and the host definitions disagree on (status or inlier count).
// Then the same for the five-point chain on the same views ("solver": "five_point" lines): T five-point subsets, the five-point kernel, the
// score kernel over the 10 T solution slots and the pick kernel alone, the whole rsba_epipolar_hypotheses_five_point call, the host chain
// (epi_detail::five_point_hypothesis) once.  -DRSBA_FIVE_LANES=64 builds the five-point kernel with 64 subsets per workgroup.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../rsba_amd/csrc/kernels_epipolar.hip"
#include "../rsba_amd/csrc/pnp_state.hpp"   // launch_pnp_normalise: the library's
#include "rsba/two_view.hpp"
#include "../rsba_amd/csrc/kernels_five_point.hip"   // (last: the file switches contraction off for what follows it)

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define CALL(x) do { int32_t r_ = (x); if (r_ != 0) { std::fprintf(stderr, "%s: %s\n", #x, rsba_last_error()); return 1; } } while (0)

struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {0.5 * (v[(v.size() - 1) / 2] + v[v.size() / 2]), v.front(), v.back()};
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main() {
  const double cam[9] = {800, 800, 0, 0, 0, 0, 0, 640, 360};
  const double pose_b[6] = {0.03, -0.05, 0.02, 0.97, 0.05, 0.24};
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  const int warm = 3, reps = 10;
  for (int n : {500, 8000}) {
    std::vector<float> xa((size_t)n * 2), xb((size_t)n * 2);
    uint64_t s = 12345;
    auto uni = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; };
    for (int i = 0; i < n; ++i) {
      const double X[3] = {-4 + 8 * uni(), -3 + 6 * uni(), 6 + 6 * uni()};
      const double d[3] = {X[0] - pose_b[3], X[1] - pose_b[4], X[2] - pose_b[5]};
      double q[3];
      rsba_amd::hyp_detail::rotate(pose_b, d, q);
      xa[2 * (size_t)i] = (float)(800 * X[0] / X[2] + 640 + uni() - 0.5); xa[2 * (size_t)i + 1] = (float)(800 * X[1] / X[2] + 360 + uni() - 0.5);
      xb[2 * (size_t)i] = (float)(800 * q[0] / q[2] + 640 + uni() - 0.5); xb[2 * (size_t)i + 1] = (float)(800 * q[1] / q[2] + 360 + uni() - 0.5);
    }
    // both sides normalised once, on the device
    double* d_n[2];
    for (int side = 0; side < 2; ++side) {
      rsba::PnpDltArgs D{};
      for (int k = 0; k < 9; ++k) D.cam[k] = cam[k];
      float* d_xy;
      CHECK(hipMalloc(&d_xy, sizeof(float) * 2 * n)); CHECK(hipMalloc(&d_n[side], sizeof(double) * 2 * n));
      CHECK(hipMemcpy(d_xy, side ? xb.data() : xa.data(), sizeof(float) * 2 * n, hipMemcpyHostToDevice));
      D.n = n; D.image_points = d_xy; D.normalised = d_n[side];
      CHECK(rsba::launch_pnp_normalise(D, nullptr));
      CHECK(hipDeviceSynchronize()); CHECK(hipFree(d_xy));
    }
    const std::vector<double> na = rsba_amd::hyp_detail::normalised_points(cam, xa.data(), n), nb = rsba_amd::hyp_detail::normalised_points(cam, xb.data(), n);
    for (int T : {1024, 16384}) {
      const std::vector<int32_t> sub = rsba_amd::hyp_detail::distinct_subsets(n, 8, T, 0x9e3779b97f4a7c15ULL);
      int32_t* d_sub; double *d_E, *d_poses; uint8_t *d_st, *d_st2; int32_t *d_inl, *d_front;
      CHECK(hipMalloc(&d_sub, sizeof(int32_t) * sub.size())); CHECK(hipMalloc(&d_E, sizeof(double) * 9 * T)); CHECK(hipMalloc(&d_poses, sizeof(double) * 6 * T));
      CHECK(hipMalloc(&d_st, T)); CHECK(hipMalloc(&d_st2, T)); CHECK(hipMalloc(&d_inl, sizeof(int32_t) * T)); CHECK(hipMalloc(&d_front, sizeof(int32_t) * 4 * T));
      CHECK(hipMemcpy(d_sub, sub.data(), sizeof(int32_t) * sub.size(), hipMemcpyHostToDevice));
      rsba::EpiEightArgs A{};
      A.n = n; A.m = 8; A.num_tasks = T; A.na = d_n[0]; A.nb = d_n[1]; A.subsets = d_sub; A.E_out = d_E; A.status = d_st;
      rsba::EpiScoreArgs S{};
      S.n = n; S.num_tasks = T; S.f2 = 800.0 * 800.0; S.thr2 = 16.0; S.na = d_n[0]; S.nb = d_n[1]; S.E = d_E; S.status_in = d_st;
      S.num_inliers = d_inl; S.num_front = d_front; S.poses_out = d_poses; S.status = d_st2;
      std::vector<double> k8, ksc, call;
      for (int rep = -warm; rep < reps; ++rep) {
        float ms8 = 0, mssc = 0;
        CHECK(hipEventRecord(e0, nullptr)); CHECK(rsba::launch_epipolar_eight_point(A, nullptr)); CHECK(hipEventRecord(e1, nullptr)); CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms8, e0, e1));
        CHECK(hipEventRecord(e0, nullptr)); CHECK(rsba::launch_epipolar_score(S, nullptr)); CHECK(hipEventRecord(e1, nullptr)); CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&mssc, e0, e1));
        if (rep >= 0) { k8.push_back(ms8); ksc.push_back(mssc); }
      }
      std::vector<double> E((size_t)T * 9), poses((size_t)T * 6); std::vector<uint8_t> st((size_t)T); std::vector<int32_t> inl((size_t)T), front((size_t)T * 4);
      for (int rep = -warm; rep < reps; ++rep) {
        const double t0 = now_ms();
        CALL(rsba_epipolar_hypotheses(0, cam, cam, xa.data(), xb.data(), n, sub.data(), 8, T, 4.0, E.data(), poses.data(), st.data(), inl.data(), front.data()));
        if (rep >= 0) call.push_back(now_ms() - t0);
      }
      // the host definitions, one thread, once
      int mismatch = 0, accepted = 0, best_dev = 0, best_host = 0;
      const double h0 = now_ms();
      for (int t = 0; t < T; ++t) {
        double e[9], p[6]; int32_t hi = 0, hf[4];
        const bool ok = rsba_amd::epi_detail::eight_point(na.data(), nb.data(), &sub[(size_t)t * 8], 8, e) &&
                        rsba_amd::epi_detail::score(na.data(), nb.data(), n, e, 800.0 * 800.0, 16.0, &hi, hf, p);
        mismatch += ok != (st[(size_t)t] != 0) || (ok && hi != inl[(size_t)t]);
        accepted += ok;
        if (ok) best_host = std::max(best_host, (int)hi);
        if (st[(size_t)t]) best_dev = std::max(best_dev, (int)inl[(size_t)t]);
      }
      const double host_ms = now_ms() - h0;
      const Stat a = stat(k8), b = stat(ksc), c = stat(call);
      std::printf("{\"subsets\": %d, \"correspondences\": %d, \"eight_point_kernel_ms\": [%.4f, %.4f, %.4f], \"score_kernel_ms\": [%.4f, %.4f, %.4f], "
                  "\"hypotheses_call_ms\": [%.4f, %.4f, %.4f], \"host_definitions_ms\": %.1f, \"accepted\": %d, \"mismatches_with_host\": %d, "
                  "\"best_inliers_device\": %d, \"best_inliers_host\": %d, \"format\": \"[median, min, max] of 10 after 3 warm-ups\"}\n",
                  T, n, a.med, a.lo, a.hi, b.med, b.lo, b.hi, c.med, c.lo, c.hi, host_ms, accepted, mismatch, best_dev, best_host);
      CHECK(hipFree(d_sub)); CHECK(hipFree(d_E)); CHECK(hipFree(d_poses)); CHECK(hipFree(d_st)); CHECK(hipFree(d_st2)); CHECK(hipFree(d_inl)); CHECK(hipFree(d_front));
    }
    for (int T : {1024, 16384}) {   // ---- the five-point chain ----
      const std::vector<int32_t> sub = rsba_amd::hyp_detail::distinct_subsets(n, 5, T, 0x9e3779b97f4a7c15ULL);
      const size_t slots = (size_t)T * 10;
      int32_t* d_sub; double *d_E, *d_poses, *d_E1, *d_p1; uint8_t *d_st, *d_slot, *d_st2, *d_st3; int32_t *d_cnt, *d_inl, *d_front, *d_inl1, *d_front1;
      CHECK(hipMalloc(&d_sub, sizeof(int32_t) * sub.size())); CHECK(hipMalloc(&d_E, sizeof(double) * 9 * slots)); CHECK(hipMalloc(&d_poses, sizeof(double) * 6 * slots));
      CHECK(hipMalloc(&d_E1, sizeof(double) * 9 * T)); CHECK(hipMalloc(&d_p1, sizeof(double) * 6 * T)); CHECK(hipMalloc(&d_st, T)); CHECK(hipMalloc(&d_slot, slots));
      CHECK(hipMalloc(&d_st2, slots)); CHECK(hipMalloc(&d_st3, T)); CHECK(hipMalloc(&d_cnt, sizeof(int32_t) * T)); CHECK(hipMalloc(&d_inl, sizeof(int32_t) * slots));
      CHECK(hipMalloc(&d_front, sizeof(int32_t) * 4 * slots)); CHECK(hipMalloc(&d_inl1, sizeof(int32_t) * T)); CHECK(hipMalloc(&d_front1, sizeof(int32_t) * 4 * T));
      CHECK(hipMemcpy(d_sub, sub.data(), sizeof(int32_t) * sub.size(), hipMemcpyHostToDevice));
      CHECK(hipMemset(d_E, 0, sizeof(double) * 9 * slots));
      rsba::EpiFiveArgs F{};
      F.n = n; F.num_tasks = T; F.na = d_n[0]; F.nb = d_n[1]; F.subsets = d_sub; F.E_out = d_E; F.num_solutions = d_cnt; F.slot_status = d_slot; F.status = d_st;
      rsba::EpiScoreArgs S{};
      S.n = n; S.num_tasks = (int)slots; S.f2 = 800.0 * 800.0; S.thr2 = 16.0; S.na = d_n[0]; S.nb = d_n[1]; S.E = d_E; S.status_in = d_slot;
      S.num_inliers = d_inl; S.num_front = d_front; S.poses_out = d_poses; S.status = d_st2;
      rsba::EpiPickArgs P{};
      P.num_tasks = T; P.slot_status = d_st2; P.slot_inliers = d_inl; P.slot_front = d_front; P.slot_E = d_E; P.slot_poses = d_poses;
      P.E_out = d_E1; P.poses_out = d_p1; P.num_inliers = d_inl1; P.num_front = d_front1; P.status = d_st3;
      std::vector<double> k5, ksc, kpick, call;
      for (int rep = -warm; rep < reps; ++rep) {
        float ms5 = 0, mssc = 0, mspick = 0;
        CHECK(hipEventRecord(e0, nullptr)); CHECK(rsba::launch_epipolar_five_point(F, nullptr)); CHECK(hipEventRecord(e1, nullptr)); CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms5, e0, e1));
        CHECK(hipEventRecord(e0, nullptr)); CHECK(rsba::launch_epipolar_score(S, nullptr)); CHECK(hipEventRecord(e1, nullptr)); CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&mssc, e0, e1));
        CHECK(hipEventRecord(e0, nullptr)); CHECK(rsba::launch_epipolar_pick(P, nullptr)); CHECK(hipEventRecord(e1, nullptr)); CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&mspick, e0, e1));
        if (rep >= 0) { k5.push_back(ms5); ksc.push_back(mssc); kpick.push_back(mspick); }
      }
      std::vector<double> E((size_t)T * 9), poses((size_t)T * 6); std::vector<uint8_t> st((size_t)T); std::vector<int32_t> inl((size_t)T), front((size_t)T * 4), cnt((size_t)T);
      for (int rep = -warm; rep < reps; ++rep) {
        const double t0 = now_ms();
        CALL(rsba_epipolar_hypotheses_five_point(0, cam, cam, xa.data(), xb.data(), n, sub.data(), T, 4.0, E.data(), poses.data(), st.data(), inl.data(), front.data(), cnt.data()));
        if (rep >= 0) call.push_back(now_ms() - t0);
      }
      int mismatch = 0, accepted = 0, best_dev = 0, best_host = 0;
      long solutions = 0;
      const double h0 = now_ms();
      for (int t = 0; t < T; ++t) {
        double e[9], p[6]; int32_t hi = 0, hf[4]; int ns = 0;
        const bool ok = rsba_amd::epi_detail::five_point_hypothesis(na.data(), nb.data(), n, &sub[(size_t)t * 5], 800.0 * 800.0, 16.0, e, p, &hi, hf, &ns);
        mismatch += ok != (st[(size_t)t] != 0) || ns != cnt[(size_t)t] || (ok && hi != inl[(size_t)t]);
        accepted += ok; solutions += ns;
        if (ok) best_host = std::max(best_host, (int)hi);
        if (st[(size_t)t]) best_dev = std::max(best_dev, (int)inl[(size_t)t]);
      }
      const double host_ms = now_ms() - h0;
      const Stat a = stat(k5), b = stat(ksc), c = stat(kpick), d = stat(call);
      std::printf("{\"solver\": \"five_point\", \"lanes_per_workgroup\": %d, \"subsets\": %d, \"correspondences\": %d, \"five_point_kernel_ms\": [%.4f, %.4f, %.4f], "
                  "\"score_kernel_ms\": [%.4f, %.4f, %.4f], \"pick_kernel_ms\": [%.4f, %.4f, %.4f], \"hypotheses_call_ms\": [%.4f, %.4f, %.4f], "
                  "\"host_definitions_ms\": %.1f, \"accepted\": %d, \"solutions\": %ld, \"mismatches_with_host\": %d, \"best_inliers_device\": %d, "
                  "\"best_inliers_host\": %d, \"format\": \"[median, min, max] of 10 after 3 warm-ups\"}\n",
                  rsba::kFiveLanes, T, n, a.med, a.lo, a.hi, b.med, b.lo, b.hi, c.med, c.lo, c.hi, d.med, d.lo, d.hi, host_ms, accepted, solutions, mismatch, best_dev, best_host);
      CHECK(hipFree(d_sub)); CHECK(hipFree(d_E)); CHECK(hipFree(d_poses)); CHECK(hipFree(d_E1)); CHECK(hipFree(d_p1)); CHECK(hipFree(d_st)); CHECK(hipFree(d_slot));
      CHECK(hipFree(d_st2)); CHECK(hipFree(d_st3)); CHECK(hipFree(d_cnt)); CHECK(hipFree(d_inl)); CHECK(hipFree(d_front)); CHECK(hipFree(d_inl1)); CHECK(hipFree(d_front1));
    }
    CHECK(hipFree(d_n[0])); CHECK(hipFree(d_n[1]));
  }
  return 0;
}
