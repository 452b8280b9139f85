// C-ABI of the descriptor matcher (include/rsba_amd.h: rsba_match_descriptors) — the k-nearest-neighbour search of
// VideoSfMClient::Match (VideoSfMClient.cc:73-129) for a list of (query frame, train frame) pairs, as parseFrame (:196-201)
// forms them.  No handle: each host thread keeps one growing device arena + pinned staging buffers + stream, as
// rsba_track_candidates does, so a call is one upload, the three passes of kernels_match.hip and one download.
#include "../../include/rsba_amd.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "capi_util.hpp"
#include "match.hpp"

using namespace rsba;

namespace {

inline size_t up16(size_t b) { return (b + 15) & ~size_t(15); }

// per host thread and device: one input block (uploaded in one copy), one output block (downloaded in one copy) and the
// scratch that never leaves the device (norms, candidate lists)
struct Arena {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float last_kernel_ms = -1.f;
  size_t in_cap = 0, out_cap = 0, tmp_cap = 0;   // bytes
  char *d_in = nullptr, *d_out = nullptr, *d_tmp = nullptr, *h_in = nullptr, *h_out = nullptr;
  void release() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_tmp); (void)hipHostFree(h_in); (void)hipHostFree(h_out);
    d_in = d_out = d_tmp = h_in = h_out = nullptr; in_cap = out_cap = tmp_cap = 0;
    if (stream) { (void)hipStreamDestroy(stream); stream = nullptr; }
    if (ev0) { (void)hipEventDestroy(ev0); ev0 = nullptr; }
    if (ev1) { (void)hipEventDestroy(ev1); ev1 = nullptr; }
  }
  // (thread_local, as the track arena: destroyed when its thread ends; errors of the frees are ignored)
  ~Arena() { release(); }
  static size_t grow(size_t have, size_t need) { size_t c = std::max<size_t>(have, 1 << 16); while (c < need) c *= 2; return c; }
  int32_t reserve(int dev, size_t in_bytes, size_t out_bytes, size_t tmp_bytes) {
    if (dev != device) { release(); device = dev; }
    RSBA_HIP_TRY(hipSetDevice(dev));
    if (!stream) RSBA_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (!ev0) RSBA_HIP_TRY(hipEventCreate(&ev0));
    if (!ev1) RSBA_HIP_TRY(hipEventCreate(&ev1));
    if (in_bytes > in_cap) {
      (void)hipFree(d_in); (void)hipHostFree(h_in); d_in = h_in = nullptr; in_cap = 0;
      const size_t c = grow(in_cap, in_bytes);
      RSBA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_in), c));
      RSBA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_in), c));
      in_cap = c;
    }
    if (out_bytes > out_cap) {
      (void)hipFree(d_out); (void)hipHostFree(h_out); d_out = h_out = nullptr; out_cap = 0;
      const size_t c = grow(out_cap, out_bytes);
      RSBA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_out), c));
      RSBA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_out), c));
      out_cap = c;
    }
    if (tmp_bytes > tmp_cap) {
      (void)hipFree(d_tmp); d_tmp = nullptr; tmp_cap = 0;
      const size_t c = grow(tmp_cap, tmp_bytes);
      RSBA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_tmp), c));
      tmp_cap = c;
    }
    return RSBA_OK;
  }
};
thread_local Arena g_arena;

struct Layout {
  size_t size = 0;
  size_t add(size_t bytes) { const size_t at = size; size = up16(size + bytes); return at; }
};

// workgroups the search aims for: a pair's train tiles are split over several workgroups while the call has fewer
constexpr int64_t kTargetItems = 1024;
constexpr int64_t kMaxSplit = 16;

}  // namespace

extern "C" int32_t rsba_match_descriptors(int32_t device, const float* desc, int32_t dim, const int64_t* frame_offset, int32_t num_frames,
                                          const int32_t* pair_query, const int32_t* pair_train, int64_t num_pairs, int32_t k,
                                          const int64_t* out_offset, int32_t* nn_index, float* nn_dist, int32_t* nn_count) {
  if (dim != MATCH_DIM) return rsba_set_error(RSBA_ERR_UNSUPPORTED, ("descriptors of " + std::to_string(dim) + " floats: only dim == 128 (SIFT, FEATURE_SIZE) is built").c_str());
  if (k < 1 || k > MATCH_KMAX) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, ("k = " + std::to_string(k) + ": k must lie in [1, 5]").c_str());
  if (num_pairs < 0 || num_frames < 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "negative count");
  if (num_pairs == 0) return RSBA_OK;
  if (!frame_offset || !pair_query || !pair_train || !out_offset || num_frames < 1) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (num_pairs > (1 << 24)) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "too many pairs for one call");
  // every offset the kernels follow is checked here
  if (frame_offset[0] != 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "frame_offset[0] != 0");
  for (int32_t f = 0; f < num_frames; ++f) {
    if (frame_offset[f + 1] < frame_offset[f]) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "frame_offset decreases");
    if (frame_offset[f + 1] - frame_offset[f] > (1 << 24)) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "a frame has more than 2^24 descriptors");
  }
  const int64_t rows = frame_offset[num_frames];
  if (rows > 0 && !desc) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");

  const int K = k <= 2 ? 2 : MATCH_KMAX;
  std::vector<MatchPair> pairs((size_t)num_pairs);
  std::vector<int64_t> qstart((size_t)num_pairs + 1, 0);
  int64_t blocks0 = 0, slots_end = 0;
  for (int64_t p = 0; p < num_pairs; ++p) {
    const int32_t fq = pair_query[p], ft = pair_train[p];
    if (fq < 0 || fq >= num_frames || ft < 0 || ft >= num_frames) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "pair refers to a frame that does not exist");
    MatchPair& P = pairs[(size_t)p];
    P.q_row = frame_offset[fq]; P.nq = (int32_t)(frame_offset[fq + 1] - frame_offset[fq]);
    P.t_row = frame_offset[ft]; P.nt = (int32_t)(frame_offset[ft + 1] - frame_offset[ft]);
    P.out = out_offset[p]; P.cand = 0; P.lists = 0; P.pad_ = 0;
    if (P.out < 0 || P.out % k != 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "out_offset must be a non-negative multiple of k");
    // pairs may come in any order, but their output ranges must not overlap: the order of out_offset decides the size of the arrays
    slots_end = std::max(slots_end, P.out + (int64_t)P.nq * k);
    qstart[(size_t)p + 1] = qstart[(size_t)p] + P.nq;
    if (P.nt >= 2) blocks0 += (P.nq + MATCH_QBLOCK - 1) / MATCH_QBLOCK;
  }
  const int64_t num_queries = qstart[(size_t)num_pairs];
  if (num_queries == 0) return RSBA_OK;
  if (!nn_index || !nn_dist || !nn_count) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (num_queries > 0x7fffffff / 8) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "too many queries for one call");
  {  // output ranges must be disjoint: a query slot written by two pairs would depend on the order of the workgroups
    std::vector<std::pair<int64_t, int64_t>> rg;
    for (const MatchPair& P : pairs) if (P.nq) rg.emplace_back(P.out, P.out + (int64_t)P.nq * k);
    std::sort(rg.begin(), rg.end());
    for (size_t i = 1; i < rg.size(); ++i) if (rg[i].first < rg[i - 1].second) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "output ranges of two pairs overlap");
  }
  int32_t rc = rsba_check_device(device);
  if (rc) return rc;

  // work items: (pair, block of 128 queries, range of train tiles)
  const int64_t split = blocks0 ? std::min<int64_t>(kMaxSplit, std::max<int64_t>(1, (kTargetItems + blocks0 - 1) / blocks0)) : 1;
  std::vector<MatchItem> items;
  int64_t lists = 0;
  for (int64_t p = 0; p < num_pairs; ++p) {
    MatchPair& P = pairs[(size_t)p];
    if (P.nt < 2 || P.nq == 0) continue;
    const int32_t tiles = (P.nt + MATCH_TTILE - 1) / MATCH_TTILE;
    const int32_t per = (int32_t)((tiles + split - 1) / split), ns = (tiles + per - 1) / per;
    P.cand = lists; P.lists = 2 * ns;
    lists += (int64_t)P.nq * P.lists;
    for (int32_t q0 = 0; q0 < P.nq; q0 += MATCH_QBLOCK)
      for (int32_t s = 0; s < ns; ++s) items.push_back(MatchItem{(int32_t)p, q0, s * per, std::min(tiles, (s + 1) * per), s, 0});
  }

  const size_t NP = (size_t)num_pairs, NI = items.size(), NS = (size_t)slots_end;
  Layout in;
  const size_t o_desc = in.add((size_t)rows * MATCH_DIM * sizeof(float)), o_pairs = in.add(NP * sizeof(MatchPair)), o_items = in.add(NI * sizeof(MatchItem)),
               o_qs = in.add((NP + 1) * sizeof(int64_t));
  Layout out;
  const size_t o_idx = out.add(NS * sizeof(int32_t)), o_dist = out.add(NS * sizeof(float)), o_cnt = out.add(NS / (size_t)k * sizeof(int32_t));
  Layout tmp;
  const size_t o_norm = tmp.add((size_t)rows * sizeof(float)), o_ckey = tmp.add((size_t)lists * K * sizeof(float)), o_cidx = tmp.add((size_t)lists * K * sizeof(int32_t));
  Arena& A = g_arena;
  if ((rc = A.reserve(device, in.size, out.size, std::max<size_t>(tmp.size, 16)))) return rc;

  if (rows) std::memcpy(A.h_in + o_desc, desc, (size_t)rows * MATCH_DIM * sizeof(float));
  std::memcpy(A.h_in + o_pairs, pairs.data(), NP * sizeof(MatchPair));
  if (NI) std::memcpy(A.h_in + o_items, items.data(), NI * sizeof(MatchItem));
  std::memcpy(A.h_in + o_qs, qstart.data(), (NP + 1) * sizeof(int64_t));
  RSBA_HIP_TRY(hipMemcpyAsync(A.d_in, A.h_in, in.size, hipMemcpyHostToDevice, A.stream));
  // The whole slot range [0, slots_end) is downloaded and handed to the caller.  Slots in gaps between the pairs' ranges are
  // written by no kernel: their index is preset to -1 (all bits set) and their count to 0 here; their DISTANCE stays
  // uninitialised device memory and is set to +inf on the host after the download, wherever the index is negative.
  RSBA_HIP_TRY(hipMemsetAsync(A.d_out, 0xff, o_dist, A.stream));
  RSBA_HIP_TRY(hipMemsetAsync(A.d_out + o_cnt, 0, NS / (size_t)k * sizeof(int32_t), A.stream));

  MatchArgs a;
  a.desc = reinterpret_cast<const float*>(A.d_in + o_desc);
  a.norm = reinterpret_cast<float*>(A.d_tmp + o_norm);
  a.pairs = reinterpret_cast<const MatchPair*>(A.d_in + o_pairs);
  a.items = reinterpret_cast<const MatchItem*>(A.d_in + o_items);
  a.rows = rows; a.num_pairs = num_pairs; a.num_items = (int64_t)NI; a.num_queries = num_queries;
  a.query_pair_start = reinterpret_cast<const int64_t*>(A.d_in + o_qs);
  a.cand_key = reinterpret_cast<float*>(A.d_tmp + o_ckey);
  a.cand_idx = reinterpret_cast<int32_t*>(A.d_tmp + o_cidx);
  a.K = K; a.k = k;
  a.nn_index = reinterpret_cast<int32_t*>(A.d_out + o_idx);
  a.nn_dist = reinterpret_cast<float*>(A.d_out + o_dist);
  a.nn_count = reinterpret_cast<int32_t*>(A.d_out + o_cnt);
  RSBA_HIP_TRY(hipEventRecord(A.ev0, A.stream));
  RSBA_HIP_TRY(launch_match(a, A.stream));
  RSBA_HIP_TRY(hipEventRecord(A.ev1, A.stream));
  RSBA_HIP_TRY(hipMemcpyAsync(A.h_out, A.d_out, out.size, hipMemcpyDeviceToHost, A.stream));
  RSBA_HIP_TRY(hipStreamSynchronize(A.stream));
  RSBA_HIP_TRY(hipEventElapsedTime(&A.last_kernel_ms, A.ev0, A.ev1));
  std::memcpy(nn_index, A.h_out + o_idx, NS * sizeof(int32_t));
  std::memcpy(nn_dist, A.h_out + o_dist, NS * sizeof(float));
  std::memcpy(nn_count, A.h_out + o_cnt, NS / (size_t)k * sizeof(int32_t));
  // (a gap's distance was never written on the device: the +inf the header promises)
  for (size_t i = 0; i < NS; ++i) if (nn_index[i] < 0) nn_dist[i] = INFINITY;
  return RSBA_OK;
}

extern "C" int32_t rsba_match_last_kernel_ms(float* ms) {
  if (!ms) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (g_arena.last_kernel_ms < 0.f) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "this thread has not run rsba_match_descriptors");
  *ms = g_arena.last_kernel_ms;
  return RSBA_OK;
}
