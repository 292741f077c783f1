// ransac_rng.h -- the host algorithms of the RANSAC driver that must match the reference bit for bit: the restatement of
// std::mt19937 with libstdc++'s distributions, the sample streams of one round (RandomSampler, PROSAC, EXHAUSTIVE, the P4Pfr
// draws) and the sequential replay of the acceptance rules.  Plain C++17, no HIP: tests/ransac_host_check.cpp runs it alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

#include "theia_hip.h"

namespace thip {

constexpr int kMaxSample = 8;            // largest minimal sample (8-point fundamental matrix)

// std::mt19937 + libstdc++ uniform_int_distribution<int> (Lemire), i.e. the
// stream RandomNumberGenerator::RandInt draws (util/random.cc:46-84).
// mt + idx are libstdc++'s _M_x + _M_p (theia_rng_state); `twists` counts regenerations, so drawn() is the number of words taken
// since the last seed (the streams driver's round accounting)
struct Mt19937 {
  uint32_t mt[624];
  int idx;
  uint64_t twists = 0;
  void seed(uint32_t s) {
    mt[0] = s;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    idx = 624;
    twists = 0;
  }
  void twist() {
    for (int i = 0; i < 624; ++i) {
      const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
      mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    idx = 0;
    twists++;
  }
  uint64_t drawn() const { return twists * 624 + (uint64_t)idx; }
  void discard(uint64_t words) {   // = std::mt19937::discard: the tempering of the skipped words is never needed
    while (words > 0) {
      if (idx >= 624) twist();
      const uint64_t k = std::min<uint64_t>(words, (uint64_t)(624 - idx));
      idx += (int)k; words -= k;
    }
  }
  uint32_t next() {
    if (idx >= 624) twist();
    uint32_t y = mt[idx++];
    y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
    return y;
  }
  // libstdc++ std::uniform_real_distribution<double>(lo, hi): generate_canonical<double, 53> = two 32-bit draws (g0 + g1 * 2^32) / 2^64
  // (nextafter(1, 0) should the quotient round to 1), then * (hi - lo) + lo -- RandomNumberGenerator::RandDouble (util/random.cc:68-72)
  double rand_double(double lo, double hi) {
    double sum = 0.0, tmp = 1.0;
    for (int k = 0; k < 2; ++k) { sum += (double)next() * tmp; tmp *= 4294967296.0; }
    double ret = sum / tmp;
    if (ret >= 1.0) ret = std::nextafter(1.0, 0.0);
    return ret * (hi - lo) + lo;
  }
  // libstdc++ std::normal_distribution<double>(mean, std_dev) on a FRESH distribution object, as RandomNumberGenerator::RandGaussian
  // makes one per call (util/random.cc:87-91): Marsaglia's polar method on two generate_canonical<double, 53> per trial, rejected
  // until 0 < r2 <= 1; the call returns the pair's y value and the saved x value dies with the object
  double rand_gaussian(double mean, double std_dev) {
    double x, y, r2;
    do {
      x = 2.0 * rand_double(0.0, 1.0) - 1.0;
      y = 2.0 * rand_double(0.0, 1.0) - 1.0;
      r2 = x * x + y * y;
    } while (r2 > 1.0 || r2 == 0.0);
    const double mult = std::sqrt(-2.0 * std::log(r2) / r2);
    return (y * mult) * std_dev + mean;
  }
  int rand_int(int lo, int hi) {
    const uint32_t urange = (uint32_t)hi - (uint32_t)lo;
    uint32_t ret;
    if (urange == 0xffffffffu) ret = next();
    else {
      const uint32_t range = urange + 1u;
      uint64_t product = (uint64_t)next() * (uint64_t)range;
      uint32_t low = (uint32_t)product;
      if (low < range) {
        const uint32_t threshold = (uint32_t)(-range) % range;
        while (low < threshold) { product = (uint64_t)next() * (uint64_t)range; low = (uint32_t)product; }
      }
      ret = (uint32_t)(product >> 32);
    }
    return (int)(ret + (uint32_t)lo);
  }
};

// sample_consensus_estimator.h:252-297
inline int compute_max_iterations(const theia_ransac_params& P, double min_sample_size, double inlier_ratio,
                                  double log_failure_prob, int total) {
  if (inlier_ratio == 1.0) return P.min_iterations;
  const int ninl = (int)(inlier_ratio * total);
  const double num_samples = P.use_Tdd_test ? min_sample_size + 1 : min_sample_size;
  double a = 1.0, b = 1.0;
  for (int i = 0; i < num_samples; ++i) { a *= ninl - i; b *= total - i; }
  const double prob_all_inliers = a / b;
  if (prob_all_inliers < std::numeric_limits<double>::epsilon()) return P.max_iterations;
  if (prob_all_inliers >= 1.0 - std::numeric_limits<double>::epsilon()) return P.min_iterations;
  const double num_iterations = log_failure_prob / std::log(1.0 - prob_all_inliers);
  return (int)std::max((double)P.min_iterations, std::min(num_iterations, (double)P.max_iterations));
}

// ProsacSampler::Sample (solvers/prosac_sampler.cc:62-128): data sorted by
// quality; the k-th sample draws m-1 points from the top n-1 and the n-th point
// (or m from the top n once T'_n < k).  The reference pushes index `n` itself,
// which is one past the end once n reaches N; that single case is clamped to N-1
// here (the reference reads out of bounds there).
inline void prosac_sample(Mt19937& rng, int N, int m, int kth, int* out) {
  double t_n = 20000.0;  // ransac_convergence_iterations_
  int n = m;
  for (int i = 0; i < m; ++i) t_n *= (double)(n - i) / (N - i);
  double t_n_prime = 1.0;
  for (int t = 1; t <= kth; ++t) {
    if (t > t_n_prime && n < N) {
      const double t_n_plus1 = (t_n * (n + 1.0)) / (n + 1.0 - m);
      t_n_prime += std::ceil(t_n_plus1 - t_n);
      t_n = t_n_plus1;
      n++;
    }
  }
  auto draw_unique = [&](int count, int hi) {
    for (int i = 0; i < count; ++i) {
      int r;
      bool dup;
      do {
        r = rng.rand_int(0, hi);
        dup = false;
        for (int q = 0; q < i; ++q) dup |= (out[q] == r);
      } while (dup);
      out[i] = r;
    }
  };
  if (t_n_prime < kth) draw_unique(m, n - 1);
  else { draw_unique(m - 1, n - 2); out[m - 1] = std::min(n, N - 1); }
}

struct ProblemState {
  Mt19937 rng;
  std::vector<int> idx;
  double best_cost;
  int max_iterations, it, n;
  bool done;
  int best_slot;
  int best_hyp = -1;          // hypothesis (chunk-local problem * B + iteration) of the best model, if set in this round
  int best_samples[kMaxSample];
  int round_iters;
  int kth;  // PROSAC sample counter
  int ex_i, ex_j;  // ExhaustiveSampler cursor (exhaustive_sampler.cc:48,61-79)
  // replay cursor inside the current round and LO-RANSAC state
  int base_it, rb, rj;
  bool round_done, best_refined;
  double pending_ratio;
  int num_lo;
  bool p4pfr_first;   // the P4Pfr solver's static generator re-seeds this problem's stream with 42 after its first sample
  int last_k;         // iterations of the last finished round
};
// streams mode only (StreamInit; kept apart so that the seeded path does not initialise it): the generator at the start of
// the current round (or at the P4Pfr re-seed inside it), the words iteration b of the round had taken since then (cum[b])
struct StreamRound {
  Mt19937 anchor;
  uint64_t anchor_drawn = 0;
  std::vector<uint64_t> cum;
};

// A problem of n data before its first round (the generator, p4pfr_first and last_k are the caller's: seeded or from a stream).
inline void problem_init(ProblemState& s, int n, int m, const theia_ransac_params& P, double log_failure_prob, bool undersized) {
  s.n = n;
  s.idx.resize(n);
  for (int i = 0; i < n; ++i) s.idx[i] = i;
  s.best_cost = std::numeric_limits<double>::max();
  s.max_iterations = P.max_iterations;
  if (P.min_inlier_ratio > 0)
    s.max_iterations = std::min(compute_max_iterations(P, m, P.min_inlier_ratio, log_failure_prob, n), P.max_iterations);
  s.it = 0; s.done = s.max_iterations <= 0 || undersized; s.best_slot = -1; s.kth = 1; s.ex_i = 0; s.ex_j = 1;
  s.base_it = 0; s.rb = 0; s.rj = 0; s.round_done = true; s.best_refined = false; s.pending_ratio = 0.0; s.num_lo = 0;
  for (int k = 0; k < kMaxSample; ++k) s.best_samples[k] = 0;
}

// The sample stream of one problem for one round of s.round_iters iterations (RandomSampler::Sample with its persistent
// permutation, PROSAC, EXHAUSTIVE) into out[B][m]; iterations beyond this problem's round are zero-filled.  sr != NULL
// (streams mode) keeps the generator at the round's start and the words every iteration took.
// P4Pfr takes three RandDouble(-0.5, 0.5) from the SAME generator after every sample (every RandomNumberGenerator object
// shares one std::mt19937, util/random.cc:46-66); the solver's static RandomNumberGenerator(42) re-seeds that generator the
// first time it runs in a process (four_point_focal_length_radial_distortion.cc:134-138).  The three draws of iteration b
// go to draws[b * draw_stride .. + 3); the caller makes the rotation of them.
inline void gen_round_problem(ProblemState& s, StreamRound* sr, int ransac_type, int m, int B, bool p4pfr, int* out,
                              double* draws, size_t draw_stride) {
  if (sr && s.round_iters > 0) { sr->anchor = s.rng; sr->anchor_drawn = s.rng.drawn(); sr->cum.resize(s.round_iters); }
  auto p4pfr_draws = [&](int b) {
    if (!p4pfr) return;
    if (s.p4pfr_first && s.it + b == 0) {
      s.rng.seed(42);
      if (sr) { sr->anchor = s.rng; sr->anchor_drawn = s.rng.drawn(); }   // (a problem ends after >= 1 iteration: past this point)
    }
    for (int k = 0; k < 3; ++k) draws[(size_t)b * draw_stride + k] = s.rng.rand_double(-0.5, 0.5);
  };
  for (int b = 0; b < s.round_iters; ++b) {
    if (ransac_type == THEIA_RANSAC_PROSAC) { prosac_sample(s.rng, s.n, m, s.kth++, out + (size_t)b * m); p4pfr_draws(b); }
    else if (ransac_type == THEIA_RANSAC_EXHAUSTIVE) {   // all pairs (i, j > i), wrapping around
      out[(size_t)b * 2] = s.ex_i; out[(size_t)b * 2 + 1] = s.ex_j;
      if (++s.ex_j >= s.n) {
        if (++s.ex_i >= s.n - 1) s.ex_i = 0;
        s.ex_j = s.ex_i + 1;
      }
    } else {
      for (int i = 0; i < m; ++i) {
        std::swap(s.idx[i], s.idx[s.rng.rand_int(i, s.n - 1)]);
        out[(size_t)b * m + i] = s.idx[i];
      }
      p4pfr_draws(b);
    }
    if (sr) sr->cum[b] = s.rng.drawn() - sr->anchor_drawn;
  }
  for (size_t e = (size_t)s.round_iters * m; e < (size_t)B * m; ++e) out[e] = 0;   // iterations beyond this problem's round
}

// The scores of one round of a chunk as the device hands them back: per hypothesis (chunk-local problem q, iteration b at
// q * B + b) the number of models and the first of them in its problem's dense order, per problem the first packed score.
struct RoundScores {
  int B;
  const int* counts;     // [cn * B]
  const int* hyp_base;   // [cn * B]
  const int* prefix;     // [cn + 1]
  const double* cost;    // packed
  const int* ninl;       // packed
  const int* samples;    // [cn * B][m]
};
// What one replay_problem call reports besides the problem's state.
struct ReplaySink {
  long long hypotheses = 0, models_scored = 0;
  bool paused = false;        // an LO event: RefineModel of model lo_slot of hypothesis lo_hyp (samples: s.best_samples) is due;
  int lo_slot = -1, lo_hyp = -1;   // the replay resumes with the next call, after replay_lo_result
};

inline void replay_begin_round(ProblemState& s) {
  s.base_it = s.it; s.rb = 0; s.rj = 0; s.round_done = s.done; s.best_hyp = -1;
}

// Sequential replay of the acceptance rules (sample_consensus_estimator.h:330-394) for chunk-local problem q over the
// round's scores, from where the problem stands (start of the round, or behind its last LO event).  With use_lo and an
// estimator whose RefineModel does something the replay pauses at each event.
inline void replay_problem(ProblemState& s, int q, int m, const RoundScores& sc, const theia_ransac_params& P,
                           double log_failure_prob, bool trivial_refine, ReplaySink& sink) {
  if (s.round_done) return;
  bool paused = false;
  // (a hypothesis interrupted by an LO event is finished even if max_iterations dropped meanwhile)
  while (!paused && s.rb < s.round_iters && (s.rj > 0 || s.base_it + s.rb < s.max_iterations)) {
    const size_t hyp = (size_t)q * sc.B + s.rb;
    const int nm = sc.counts[hyp];
    if (s.rj == 0) sink.hypotheses++;
    while (s.rj < nm) {
      const int j = s.rj++;
      const size_t at = (size_t)sc.prefix[q] + (size_t)sc.hyp_base[hyp] + (size_t)j;
      const double cost = sc.cost[at];
      const int ninl = sc.ninl[at];
      sink.models_scored++;
      const double inlier_ratio = (double)ninl / (double)s.n;
      if (cost < s.best_cost) {
        s.best_cost = cost;
        s.best_slot = j;
        s.best_hyp = (int)hyp;
        s.best_refined = false;
        for (int i = 0; i < m; ++i) s.best_samples[i] = sc.samples[hyp * m + i];
        if (inlier_ratio < m / (double)s.n) continue;
        if (P.use_lo && trivial_refine && s.base_it + s.rb >= P.lo_start_iterations) {
          s.num_lo++;   // RefineModel = "return true": nothing changes but the counter
        } else if (P.use_lo && s.base_it + s.rb >= P.lo_start_iterations) {   // :373-381
          sink.paused = true; sink.lo_slot = j; sink.lo_hyp = (int)hyp;
          s.pending_ratio = inlier_ratio;
          paused = true;
          break;
        }
        s.max_iterations = std::min(compute_max_iterations(P, m, inlier_ratio, log_failure_prob, s.n), s.max_iterations);
      }
    }
    if (!paused) { s.rb++; s.rj = 0; }
  }
  if (!paused) {
    s.round_done = true;
    s.it = s.base_it + s.rb;
    s.last_k = s.rb;
    if (s.it >= s.max_iterations) s.done = true;
  }
}

// the outcome of the RefineModel a replay paused for
inline void replay_lo_result(ProblemState& s, int m, bool ok, const theia_ransac_params& P, double log_failure_prob) {
  s.best_refined = true;                       // RefineModel overwrites the pose even when it fails
  if (!ok) return;                             // "continue": no max_iterations update
  s.num_lo++;
  s.max_iterations = std::min(compute_max_iterations(P, m, s.pending_ratio, log_failure_prob, s.n), s.max_iterations);
}

}  // namespace thip
