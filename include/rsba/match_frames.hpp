// Descriptor matching on a Session: the step that fills Observation::matches.
//   VideoSfMClient::Match        /root/reference/src/rsba/VideoSfMClient.cc:73-129  (calc2Ddist :57-69)
//   the loop of parseFrame       /root/reference/src/rsba/VideoSfMClient.cc:196-201
//   convertCV(obs, matches, key) /root/reference/src/rsba/struct/VideoSfM.cc:48-54
// Match is a brute-force k-nearest-neighbour search over the frames' 128-float SIFT descriptors (cv::BFMatcher, NORM_L2;
// k = 2, or 5 with `multiple`) followed by a ratio test and a 2-D displacement filter.  The search — n_query x n_train x 128
// multiply-adds per pair — runs on the device (rsba_match_descriptors, whose header comment defines the neighbour order);
// the filter is O(n), needs a SEQUENTIAL double sum over the queries (std::accumulate, :94) and stays on the host, in the
// reference's arithmetic:
//   calc2Ddist   dx = double(float(x_q) - float(x_t)) — the subtraction is in float, key points are cv::Point2f — likewise dy,
//                then sqrt(dx * dx + dy * dy) in double
//   threshold    mean + mean, mean = (the sum of every query's best neighbour's 2-D distance, in query order) / n_query
//   default      ms[0] is kept iff ms[0].distance < ratio * ms[1].distance (float product, float compare; ratio = 0.80f, so
//                distances 4 and 5 are REJECTED: 0.8f * 5.0f rounds to 4.0f) and its 2-D distance < threshold
//   multiple     as written in the reference: ms[0] is kept iff its 2-D distance passes (no ratio test); ms[i], i >= 1, iff
//                ms[0].distance > ratio * ms[1].distance and its own 2-D distance passes
// Output order: query order, then neighbour order.  A pair with n_train < 2 (the reference reads ms[1] out of bounds) or
// n_query == 0 (it divides by zero) yields no matches.
// A missing device throws std::runtime_error; filterMatches needs none.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../rsba_amd.h"
#include "session.hpp"

namespace rsba_amd {

constexpr int FEATURE_SIZE = 128;   // struct/VideoSfM.cc:11-13

struct DMatch {           // cv::DMatch, the members Match uses
  int32_t queryIdx = 0, trainIdx = 0;
  float distance = 0;
};

namespace match_detail {
inline double dist2D(const double* q, const double* t) {   // calc2Ddist (:57-69)
  const float qx = (float)q[0], qy = (float)q[1], tx = (float)t[0], ty = (float)t[1];
  const float fx = qx - tx, fy = qy - ty;
  const double dx = fx, dy = fy;
  return std::sqrt(dx * dx + dy * dy);
}
}  // namespace match_detail

// The filter of Match (:85-128) on a kNN result in the layout of rsba_match_descriptors: k slots per query (index within the
// train frame, distance), nn_count[i] of them used.  xy_query [n_query][2], xy_train [n_train][2].
inline std::vector<DMatch> filterMatches(const int32_t* nn_index, const float* nn_dist, const int32_t* nn_count, size_t n_query, int k,
                                         const double* xy_query, const double* xy_train, bool multiple) {
  std::vector<DMatch> good;
  if (n_query == 0) return good;
  for (size_t i = 0; i < n_query; ++i) if (nn_count[i] < 2) return good;   // n_train < 2
  const float ratio = 0.80f;
  auto d2 = [&](size_t i, int n) { return match_detail::dist2D(xy_query + 2 * i, xy_train + 2 * (size_t)nn_index[i * (size_t)k + (size_t)n]); };
  double sum = 0.0;
  for (size_t i = 0; i < n_query; ++i) sum += d2(i, 0);
  const double mean = sum / (double)n_query;
  const double threshold = mean + mean;
  for (size_t i = 0; i < n_query; ++i) {
    const float* dist = nn_dist + i * (size_t)k;
    const int32_t* idx = nn_index + i * (size_t)k;
    const float bound = ratio * dist[1];
    if (multiple) {
      if (d2(i, 0) < threshold) good.push_back(DMatch{(int32_t)i, idx[0], dist[0]});
      for (int n = 1; n < nn_count[i]; ++n)
        if (dist[0] > bound && d2(i, n) < threshold) good.push_back(DMatch{(int32_t)i, idx[n], dist[n]});
    } else {
      if (dist[0] < bound && d2(i, 0) < threshold) good.push_back(DMatch{(int32_t)i, idx[0], dist[0]});
    }
  }
  return good;
}

namespace match_detail {

// One device call for a list of (query frame, train frame) pairs of a session, then the filter per pair.
inline std::vector<std::vector<DMatch>> run(const Session& sess, const std::vector<std::pair<size_t, size_t>>& pairs, bool multiple, int device) {
  std::vector<std::vector<DMatch>> kept(pairs.size());
  if (pairs.empty()) return kept;
  // the frames the pairs name, each uploaded once
  std::vector<int32_t> slot(sess.frames.size(), -1);
  std::vector<size_t> used;
  for (const auto& p : pairs)
    for (size_t f : {p.first, p.second}) {
      if (f >= sess.frames.size()) throw std::runtime_error("Match: frame " + std::to_string(f) + " does not exist");
      if (slot[f] < 0) { slot[f] = (int32_t)used.size(); used.push_back(f); }
    }
  std::vector<int64_t> frame_offset(used.size() + 1, 0);
  for (size_t u = 0; u < used.size(); ++u) frame_offset[u + 1] = frame_offset[u] + (int64_t)sess.frames[used[u]].obs.size();
  std::vector<float> desc((size_t)frame_offset.back() * FEATURE_SIZE);
  const size_t bytes = FEATURE_SIZE * sizeof(float);
  for (size_t u = 0; u < used.size(); ++u) {
    const Frame& f = sess.frames[used[u]];
    for (size_t i = 0; i < f.obs.size(); ++i) {
      if (f.obs[i].descriptor.size() != bytes)
        throw std::runtime_error("Match: observation " + std::to_string(i) + " of frame " + std::to_string(used[u]) + " has no " + std::to_string(bytes) + "-byte descriptor");
      std::memcpy(desc.data() + ((size_t)frame_offset[u] + i) * FEATURE_SIZE, f.obs[i].descriptor.data(), bytes);
    }
  }
  const int k = multiple ? 5 : 2;
  std::vector<int32_t> pq(pairs.size()), pt(pairs.size());
  std::vector<int64_t> out(pairs.size() + 1, 0);
  for (size_t p = 0; p < pairs.size(); ++p) {
    pq[p] = slot[pairs[p].first]; pt[p] = slot[pairs[p].second];
    out[p + 1] = out[p] + (int64_t)k * (int64_t)sess.frames[pairs[p].first].obs.size();
  }
  const size_t slots = (size_t)out.back();
  std::vector<int32_t> nn_index(slots + 1), nn_count(slots / (size_t)k + 1);
  std::vector<float> nn_dist(slots + 1);
  if (rsba_match_descriptors(device, desc.data(), FEATURE_SIZE, frame_offset.data(), (int32_t)used.size(), pq.data(), pt.data(), (int64_t)pairs.size(), k,
                             out.data(), nn_index.data(), nn_dist.data(), nn_count.data()) != RSBA_OK)
    throw std::runtime_error(std::string("rsba_amd: ") + rsba_last_error());
  std::vector<double> xq, xt;
  for (size_t p = 0; p < pairs.size(); ++p) {
    const Frame& fq = sess.frames[pairs[p].first];
    const Frame& ft = sess.frames[pairs[p].second];
    if (fq.obs.empty() || ft.obs.size() < 2) continue;
    xq.resize(2 * fq.obs.size()); xt.resize(2 * ft.obs.size());
    for (size_t i = 0; i < fq.obs.size(); ++i) { xq[2 * i] = fq.obs[i].x; xq[2 * i + 1] = fq.obs[i].y; }
    for (size_t i = 0; i < ft.obs.size(); ++i) { xt[2 * i] = ft.obs[i].x; xt[2 * i + 1] = ft.obs[i].y; }
    kept[p] = filterMatches(nn_index.data() + out[p], nn_dist.data() + out[p], nn_count.data() + out[p] / k, fq.obs.size(), k, xq.data(), xt.data(), multiple);
  }
  return kept;
}

// convertCV(f.obs, matches, trainFrame) (struct/VideoSfM.cc:48-54)
inline void append(Frame& f, const std::vector<DMatch>& matches, size_t trainFrame) {
  for (const DMatch& m : matches) {
    Observation& o = f.obs[(size_t)m.queryIdx];
    ObservationRef ref;
    ref.frame = (int32_t)trainFrame; ref.obs = m.trainIdx; ref.valid = false;
    o.matches.push_back(ref);
    o.__isset.matches = true;
  }
}

inline std::vector<std::pair<size_t, size_t>> frame_pairs(size_t frameKey, const SfmOptions& opt) {
  std::vector<std::pair<size_t, size_t>> pairs;
  for (size_t i = 1; i <= frameKey && i <= opt.tracks.maxFramesToMatch; ++i) pairs.emplace_back(frameKey, frameKey - i);   // :196
  return pairs;
}

}  // namespace match_detail

// VideoSfMClient::Match(descriptors of queryFrame, of trainFrame, their key points, multiple): one device call + the filter.
inline std::vector<DMatch> Match(const Session& sess, size_t queryFrame, size_t trainFrame, bool multiple = false, int device = 0) {
  return match_detail::run(sess, {{queryFrame, trainFrame}}, multiple, device)[0];
}

// The matching loop of parseFrame (:196-201) for one frame: frame frameKey against frames frameKey - 1 ... frameKey - maxFramesToMatch
// in ONE device call; the kept matches are appended to the query observations in that order (valid = false).  parseFrame
// itself always matches with multiple == false.  Throws when an observation of an involved frame has no 512-byte descriptor.
inline void matchFrame(Session& sess, size_t frameKey, const SfmOptions& opt, bool multiple = false, int device = 0) {
  if (frameKey >= sess.frames.size()) throw std::runtime_error("matchFrame: frame " + std::to_string(frameKey) + " does not exist");
  const auto pairs = match_detail::frame_pairs(frameKey, opt);
  const auto kept = match_detail::run(sess, pairs, multiple, device);
  for (size_t p = 0; p < pairs.size(); ++p) match_detail::append(sess.frames[frameKey], kept[p], pairs[p].second);
}

// Every frame of the session in ONE device call: the result of matchFrame for frameKey = 1 ... F - 1 (matching reads
// descriptors and positions only, never the matches of earlier frames).
inline void matchSession(Session& sess, const SfmOptions& opt, bool multiple = false, int device = 0) {
  std::vector<std::pair<size_t, size_t>> pairs;
  for (size_t fk = 1; fk < sess.frames.size(); ++fk) {
    const auto fp = match_detail::frame_pairs(fk, opt);
    pairs.insert(pairs.end(), fp.begin(), fp.end());
  }
  const auto kept = match_detail::run(sess, pairs, multiple, device);
  for (size_t p = 0; p < pairs.size(); ++p) match_detail::append(sess.frames[pairs[p].first], kept[p], pairs[p].second);
}

}  // namespace rsba_amd
