// Arguments of the descriptor-matching kernels (kernels_match.hip), staged by match_capi.hip.  Every offset has been checked on
// the host before the launch: a pair's query / train rows lie inside desc, its output slots inside nn_*, its candidate lists
// inside cand_*.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsba {

constexpr int MATCH_DIM = 128;      // FEATURE_SIZE (struct/VideoSfM.cc:11-13)
constexpr int MATCH_QBLOCK = 128;   // queries of one workgroup: 4 waves x 32 lanes' columns
constexpr int MATCH_TTILE = 128;    // train rows of one LDS tile: 4 accumulators x 32 rows per wave
constexpr int MATCH_KMAX = 5;

struct MatchPair {      // one (query frame, train frame) pair
  int64_t q_row, t_row;   // first descriptor row of the query / train frame in desc
  int64_t out;            // first output slot (k per query)
  int64_t cand;           // first candidate list of the pair: query i's lists are cand + i * lists .. + lists - 1
  int32_t nq, nt;
  int32_t lists;          // partial top-K lists per query = 2 (lane halves) x train splits
  int32_t pad_;
};

struct MatchItem {      // one workgroup of the search: a block of queries against a range of train tiles
  int32_t pair, q0, tile0, tile1, split, pad_;
};

struct MatchArgs {
  const float* desc;        // [rows][128]
  float* norm;              // [rows]  ||row||^2 (written by the norm pass)
  const MatchPair* pairs;
  const MatchItem* items;
  int64_t rows, num_pairs, num_items, num_queries;
  const int64_t* query_pair_start;   // [num_pairs + 1] prefix sum of nq: the refine pass finds its pair by bisection
  float* cand_key;          // [lists][K] search distances sqrtf(d2), ascending
  int32_t* cand_idx;        // [lists][K]
  int32_t K;                // 2 or 5: the width of the lists (>= k)
  int32_t k;                // what the caller asked for
  int32_t* nn_index; float* nn_dist; int32_t* nn_count;
};

hipError_t launch_match(const MatchArgs& a, hipStream_t st);

}  // namespace rsba
