// ransac_streams.hip -- RANSAC on the caller's generator streams: theia_hip_ransac_estimate_streams (waves of the batch driver
// of ransac.hip, every problem starting where its stream stands) and the theia_hip_rng_* / theia_hip_randint_stream draws
// from a theia_rng_state (Mt19937, ransac_rng.h).  No kernels.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ransac_internal.h"

using namespace thip;

static bool rng_state_ok(const theia_rng_state* st) { return st && st->pos >= 0 && st->pos <= 624; }
static void rng_load(Mt19937& g, const theia_rng_state& st) {
  std::memcpy(g.mt, st.mt, sizeof(g.mt)); g.idx = st.pos; g.twists = 0;
}
static void rng_store(theia_rng_state& st, const Mt19937& g) { std::memcpy(st.mt, g.mt, sizeof(g.mt)); st.pos = g.idx; }

extern "C" {

// Every problem of one stream is an Estimate() call that starts where the previous one of its stream stopped, so the k-th
// problems of all streams ("wave" k) are independent of each other and run as one call of the batch driver; wave k + 1
// starts from the states wave k handed back.  A wave's problems are contiguous in the batch when the streams are
// interleaved (or one problem each); otherwise their data are gathered.
int theia_hip_ransac_estimate_streams(const theia_ransac_batch* batch, const theia_ransac_params* params,
                                      const theia_ransac_streams* streams, theia_ransac_result* result) {
  if (!batch || !params || !streams || !result) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (batch->seeds) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the streams entry point draws from the caller's generators: batch->seeds must be NULL");
  const int nprob = batch->num_problems, ns = streams->num_streams;
  if (nprob < 0 || (nprob > 0 && (!batch->offsets || !batch->data))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad batch");
  if (ns < 1 || !streams->states) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "streams: num_streams >= 1 and a states array are needed");
  for (int k = 0; k < ns; ++k) {
    if (!rng_state_ok(&streams->states[k])) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "stream %d: pos outside [0, 624]", k);
    if (streams->states[k].dls_calls < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "stream %d: dls_calls < 0", k);
  }
  int rc = check_result_arrays(nprob, result);
  if (rc) return rc;
  std::vector<int> sid(nprob, 0), rank(nprob, 0), count(ns, 0);
  for (int p = 0; p < nprob; ++p) {
    const int k = streams->stream_of_problem ? streams->stream_of_problem[p] : 0;
    if (k < 0 || k >= ns) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %d: stream id %d outside [0, %d)", p, k, ns);
    if (batch->offsets[p + 1] - batch->offsets[p] <= 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "Cannot perform estimation with 0 data measurements!");
    sid[p] = k; rank[p] = count[k]++;
  }
  const int est = batch->estimator;
  const bool dls_est = est == THEIA_EST_ABSOLUTE_POSE_DLS || est == THEIA_EST_SIMILARITY_2D3D;
  const bool p4pfr_est = est == THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE;
  double p4pfr_params[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // the four limits; the first-call flag comes from the streams
  if (p4pfr_est && batch->estimator_params) std::memcpy(p4pfr_params, batch->estimator_params, sizeof(double) * 4);
  theia_ransac_batch sub = *batch;
  if (p4pfr_est && batch->estimator_params) sub.estimator_params = p4pfr_params;
  if (nprob == 0) { sub.num_problems = 0; return ransac_run(&sub, params, result, nullptr); }   // (the parameter checks)
  const int ds = (est >= 0 && est <= THEIA_EST_CAMERA_ALIGNMENT) ? datum_size(est) : 1;

  // the streams, worked on in copies: the caller's states change only when every wave succeeded
  std::vector<Mt19937> gen(ns);
  std::vector<uint8_t> first(ns);   // the P4Pfr solver's static generator has not run on this stream yet
  std::vector<int64_t> dls_calls(ns);
  std::vector<dls::GlibcRand> dls_gen(dls_est ? ns : 0);
  for (int k = 0; k < ns; ++k) {
    rng_load(gen[k], streams->states[k]);
    first[k] = streams->states[k].p4pfr_static_seeded == 0;
    dls_calls[k] = streams->states[k].dls_calls;
    if (dls_est)
      for (int64_t i = 0; i < 4 * dls_calls[k]; ++i) (void)dls_gen[k].next();
  }
  const int nwaves = *std::max_element(count.begin(), count.end());
  std::vector<std::vector<int>> waves(nwaves);
  for (int p = 0; p < nprob; ++p) waves[rank[p]].push_back(p);

  reset_counters(result);
  constexpr int kS = THEIA_RANSAC_MODEL_STRIDE;
  std::vector<int64_t> off;
  std::vector<double> gathered;
  std::vector<int> wsid;
  std::vector<int32_t> r_succ, r_ninl, r_nit, r_nlo;
  std::vector<double> r_models, r_conf;
  std::vector<uint8_t> r_mask;
  for (const std::vector<int>& W : waves) {
    const int nw = (int)W.size(), p0 = W[0];
    bool contiguous = true;
    for (int i = 1; i < nw; ++i) contiguous &= W[i] == p0 + i;
    off.assign(nw + 1, 0);
    for (int i = 0; i < nw; ++i) off[i + 1] = off[i] + (batch->offsets[W[i] + 1] - batch->offsets[W[i]]);
    const double* data = batch->data + (size_t)batch->offsets[p0] * ds;
    theia_ransac_result r{};
    if (contiguous) {   // the wave's slice of the batch: data and results in place
      r.success = result->success + p0; r.models = result->models + (size_t)p0 * kS; r.num_inliers = result->num_inliers + p0;
      r.inlier_mask = result->inlier_mask + batch->offsets[p0]; r.num_iterations = result->num_iterations + p0;
      r.confidence = result->confidence + p0; r.num_lo_iterations = result->num_lo_iterations ? result->num_lo_iterations + p0 : nullptr;
    } else {
      gathered.resize((size_t)off[nw] * ds);
      for (int i = 0; i < nw; ++i)
        std::memcpy(gathered.data() + (size_t)off[i] * ds, batch->data + (size_t)batch->offsets[W[i]] * ds, sizeof(double) * (size_t)(off[i + 1] - off[i]) * ds);
      data = gathered.data();
      r_succ.assign(nw, 0); r_ninl.assign(nw, 0); r_nit.assign(nw, 0); r_nlo.assign(nw, 0);
      r_models.assign((size_t)nw * kS, 0.0); r_conf.assign(nw, 0.0); r_mask.assign((size_t)off[nw], 0);
      r.success = r_succ.data(); r.models = r_models.data(); r.num_inliers = r_ninl.data(); r.inlier_mask = r_mask.data();
      r.num_iterations = r_nit.data(); r.confidence = r_conf.data(); r.num_lo_iterations = r_nlo.data();
    }
    wsid.resize(nw);
    for (int i = 0; i < nw; ++i) wsid[i] = sid[W[i]];
    sub.num_problems = nw; sub.offsets = off.data(); sub.data = data; sub.seeds = nullptr;
    const StreamInit si{gen.data(), wsid.data(), first.data(), dls_est ? dls_gen.data() : nullptr};
    rc = ransac_run(&sub, params, &r, &si);   // (advances gen[] of the wave's streams)
    if (rc) return rc;
    if (!contiguous) {
      for (int i = 0; i < nw; ++i) {
        const int p = W[i];
        result->success[p] = r_succ[i]; result->num_inliers[p] = r_ninl[i]; result->num_iterations[p] = r_nit[i];
        result->confidence[p] = r_conf[i];
        if (result->num_lo_iterations) result->num_lo_iterations[p] = r_nlo[i];
        std::memcpy(result->models + (size_t)p * kS, r_models.data() + (size_t)i * kS, sizeof(double) * kS);
        std::memcpy(result->inlier_mask + batch->offsets[p], r_mask.data() + off[i], (size_t)(off[i + 1] - off[i]));
      }
    }
    for (int i = 0; i < nw; ++i) {
      const int k = wsid[i], nit = r.num_iterations[i];
      if (nit > 0) {   // (an undersized problem leaves its stream as it was)
        if (p4pfr_est) first[k] = 0;
        if (dls_est) {
          dls_calls[k] += nit;
          for (int64_t j = 0; j < 4 * (int64_t)nit; ++j) (void)dls_gen[k].next();
        }
      }
    }
    result->hypotheses_evaluated += r.hypotheses_evaluated; result->models_scored += r.models_scored;
    result->time_fit_score_seconds += r.time_fit_score_seconds;
    result->time_fit_seconds += r.time_fit_seconds; result->time_score_seconds += r.time_score_seconds;
  }
  for (int k = 0; k < ns; ++k) {
    theia_rng_state& st = streams->states[k];
    rng_store(st, gen[k]);
    if (p4pfr_est) st.p4pfr_static_seeded = !first[k];
    st.dls_calls = dls_calls[k];
  }
  return 0;
}

int theia_hip_rng_seed(theia_rng_state* state, uint32_t seed) {
  if (!state) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null state");
  Mt19937 g;
  g.seed(seed);
  rng_store(*state, g);
  return 0;
}

int theia_hip_rng_rand_int(theia_rng_state* state, int32_t lo, int32_t hi, int32_t n, int32_t* out) {
  if (!rng_state_ok(state)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null state or pos outside [0, 624]");
  if (n < 0 || (n > 0 && !out) || lo > hi) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  Mt19937 g;
  rng_load(g, *state);
  for (int32_t i = 0; i < n; ++i) out[i] = g.rand_int(lo, hi);
  rng_store(*state, g);
  return 0;
}

int theia_hip_rng_rand_double(theia_rng_state* state, double lo, double hi, int32_t n, double* out) {
  if (!rng_state_ok(state)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null state or pos outside [0, 624]");
  if (n < 0 || (n > 0 && !out) || !(lo <= hi)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  Mt19937 g;
  rng_load(g, *state);
  for (int32_t i = 0; i < n; ++i) out[i] = g.rand_double(lo, hi);
  rng_store(*state, g);
  return 0;
}

int theia_hip_rng_rand_gaussian(theia_rng_state* state, double mean, double std_dev, int32_t n, double* out) {
  if (!rng_state_ok(state)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null state or pos outside [0, 624]");
  if (n < 0 || (n > 0 && !out)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  Mt19937 g;
  rng_load(g, *state);
  for (int32_t i = 0; i < n; ++i) out[i] = g.rand_gaussian(mean, std_dev);
  rng_store(*state, g);
  return 0;
}

int theia_hip_rng_discard(theia_rng_state* state, uint64_t words) {
  if (!rng_state_ok(state)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null state or pos outside [0, 624]");
  Mt19937 g;
  rng_load(g, *state);
  g.discard(words);
  rng_store(*state, g);
  return 0;
}
// n draws of RandomNumberGenerator(seed).RandInt(lo, hi) (util/random.cc:46-84: std::mt19937 + uniform_int_distribution<int>), for
// host code that has to follow the reference's generator outside the sampler (the random candidates of the guided matcher)
int theia_hip_randint_stream(uint32_t seed, int32_t n, int32_t lo, int32_t hi, int32_t* out) {
  if (n < 0 || hi < lo || (n > 0 && !out)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  Mt19937 g;
  g.seed(seed);
  for (int i = 0; i < n; ++i) out[i] = g.rand_int(lo, hi);
  return 0;
}
}  // extern "C"
