// Wall time of solveGsPnPRansac (include/rsba/solve_rs_pnp.hpp) with hypotheses_on_device off (host DLT loop, then one rsba_pnp_tasks
// call) and on (one rsba_pnp_gs_hypotheses call), for 500, 1 000 and 16 384 subsets of 2 000 points; the two alternate, best and mean of
// 7 after a warm-up.  tools/pnp_dlt_time.py builds and runs this.  One JSON line per size.
#include <chrono>
#include <cmath>
#include <cstdio>

#include "pnp_time_scene.hpp"
#include "rsba/solve_rs_pnp.hpp"

int main() {
  const int n = 2000;
  const PnpTimeScene sc(n);
  for (int T : {500, 1000, 16384}) {
    double best[2] = {1e30, 1e30}, sum[2] = {0, 0}, pose[2][6]; int found[2] = {0, 0};
    const int reps = 7;
    for (int rep = -1; rep < reps; ++rep)
      for (int on = 0; on < 2; ++on) {
        const auto t0 = std::chrono::steady_clock::now();
        found[on] = rsba_amd::solveGsPnPRansac(sc.X.data(), sc.xy.data(), n, sc.cam, pose[on], T, 6.0f, 6, 0x9e3779b97f4a7c15ULL, 0, on != 0);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rep >= 0) { best[on] = std::fmin(best[on], ms); sum[on] += ms; }
      }
    double diff = 0.0;
    for (int k = 0; k < 6; ++k) diff = std::fmax(diff, std::fabs(pose[0][k] - pose[1][k]));
    std::printf("{\"subsets\": %d, \"points\": %d, \"gs_ransac_wall_ms_flag_off_min\": %.3f, \"gs_ransac_wall_ms_flag_off_mean\": %.3f, "
                "\"gs_ransac_wall_ms_flag_on_min\": %.3f, \"gs_ransac_wall_ms_flag_on_mean\": %.3f, \"inliers_off\": %d, \"inliers_on\": %d, \"pose_difference\": %.3g}\n",
                T, n, best[0], sum[0] / reps, best[1], sum[1] / reps, found[0], found[1], diff);
  }
  return 0;
}
