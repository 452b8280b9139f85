// Descriptor matching on a Session cache (include/rsba/match_frames.hpp):
//   match_frames match <session.cache> [--multiple] [--per-frame] [out.cache]
//       loads the cache WITH its descriptors, runs matchSession (one device call for the whole session) or, with --per-frame,
//       matchFrame for frameKey = 1 .. F - 1, and prints every observation's matches as JSON:
//       {"frames":[[[[frame,obs],...] per observation] per frame]}.  With out.cache the matched session is saved too (without
//       descriptors), ready for examples/create_tracks.
//   match_frames filter <file>
//       runs filterMatches alone — no device call — on a kNN result read from <file> (little endian): int64 n_query, n_train, k,
//       multiple; double xy_query[n_query][2], xy_train[n_train][2]; int32 index[n_query][k]; float distance[n_query][k];
//       int32 count[n_query].  Prints the kept matches as JSON [[queryIdx,trainIdx],...].
//   match_frames copy <in.cache> <out.cache>        load and save a session, both WITH descriptors
//   match_frames descriptors <session.cache>       prints every observation's descriptor as a hex string, per frame (JSON)
//   exit status: 0 done, 2 bad input, 3 the matcher threw (message on stderr)
#include <cstdio>
#include <cstring>
#include <string>

#include "rsba/match_frames.hpp"
#include "rsba/session_cache.hpp"

using namespace rsba_amd;

template <class T>
static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int filter(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  int64_t hd[4];
  if (std::fread(hd, sizeof(int64_t), 4, f) != 4 || hd[0] < 0 || hd[1] < 0 || hd[2] < 1 || hd[2] > 5) { std::fprintf(stderr, "bad header\n"); std::fclose(f); return 2; }
  const size_t nq = (size_t)hd[0], nt = (size_t)hd[1], k = (size_t)hd[2];
  std::vector<double> xq(2 * nq), xt(2 * nt);
  std::vector<int32_t> idx(nq * k), cnt(nq);
  std::vector<float> dist(nq * k);
  const bool ok = rd(f, xq) && rd(f, xt) && rd(f, idx) && rd(f, dist) && rd(f, cnt);
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "truncated file\n"); return 2; }
  for (size_t i = 0; i < nq; ++i) {
    if (cnt[i] < 0 || (size_t)cnt[i] > k) { std::fprintf(stderr, "bad count\n"); return 2; }
    for (int32_t n = 0; n < cnt[i]; ++n) if (idx[i * k + (size_t)n] < 0 || (size_t)idx[i * k + (size_t)n] >= nt) { std::fprintf(stderr, "index out of range\n"); return 2; }
  }
  const std::vector<DMatch> good = filterMatches(idx.data(), dist.data(), cnt.data(), nq, (int)k, xq.data(), xt.data(), hd[3] != 0);
  std::printf("[");
  for (size_t i = 0; i < good.size(); ++i) std::printf("%s[%d,%d]", i ? "," : "", good[i].queryIdx, good[i].trainIdx);
  std::printf("]\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "filter")) return filter(argv[2]);
  if ((argc == 4 && !std::strcmp(argv[1], "copy")) || (argc == 3 && !std::strcmp(argv[1], "descriptors"))) {
    Session s;
    try { loadCache(argv[2], s, true); if (argc == 4) { saveCache(argv[3], s, true); return 0; } } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
    std::printf("[");
    for (size_t fi = 0; fi < s.frames.size(); ++fi) {
      std::printf("%s[", fi ? "," : "");
      for (size_t i = 0; i < s.frames[fi].obs.size(); ++i) {
        std::printf("%s\"", i ? "," : "");
        for (unsigned char c : s.frames[fi].obs[i].descriptor) std::printf("%02x", c);
        std::printf("\"");
      }
      std::printf("]");
    }
    std::printf("]\n");
    return 0;
  }
  if (argc < 3 || std::strcmp(argv[1], "match")) {
    std::fprintf(stderr, "usage: %s match <session.cache> [--multiple] [--per-frame] [out.cache]   (out.cache: the matched session, saved without descriptors)\n"
                         "       %s filter <file>                         (the host filter alone on a kNN result; no device)\n"
                         "       %s copy <in.cache> <out.cache>           (load and save with descriptors)\n"
                         "       %s descriptors <session.cache>           (the descriptors as hex strings)\n", argv[0], argv[0], argv[0], argv[0]);
    return 2;
  }
  bool multiple = false, per_frame = false;
  const char* out = nullptr;
  for (int i = 3; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--multiple")) multiple = true;
    else if (!std::strcmp(argv[i], "--per-frame")) per_frame = true;
    else out = argv[i];
  }
  Session sess;
  try { loadCache(argv[2], sess, true); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
  SfmOptions opt;
  try {
    if (per_frame) for (size_t fk = 1; fk < sess.frames.size(); ++fk) matchFrame(sess, fk, opt, multiple);
    else matchSession(sess, opt, multiple);
    if (out) saveCache(out, sess);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  std::printf("{\"frames\":[");
  for (size_t fi = 0; fi < sess.frames.size(); ++fi) {
    std::printf("%s[", fi ? "," : "");
    const Frame& f = sess.frames[fi];
    for (size_t i = 0; i < f.obs.size(); ++i) {
      std::printf("%s[", i ? "," : "");
      for (size_t m = 0; m < f.obs[i].matches.size(); ++m) std::printf("%s[%d,%d]", m ? "," : "", f.obs[i].matches[m].frame, f.obs[i].matches[m].obs);
      std::printf("]");
    }
    std::printf("]");
  }
  std::printf("]}\n");
  return 0;
}
