// sim3_alignment.hip -- OptimizeAlignmentSim3 (sfm/transformation/align_point_clouds.cc:161-284, alignment_error.h) and the
// Sim(3) conversions (:288-317, transformation_wrapper.cc:125-132): theia_hip_optimize_alignment_sim3 and theia_hip_sim3_maps.
// The per-thread arithmetic of the maps is sim3_device.h; the step rules are lm_rules.h (the thirteenth loop on them).  This
// file must be compiled without FMA contraction (build.sh's default).  DESIGN.md 3.6v.
//
// One pass over a problem's points at the tangent a sums 36 numbers: sum rho(|r|^2), J'r (7) and the packed lower triangle of
// J'J (28).  Sim3::exp(a) and its derivative are formed ONCE per pass (lane 0 -> the 96-double table T) and every point reads
// them: r_i = w_i (y_i - (sR x_i + t)), J_i = -w_i (d(sR) x_i + dt); POINT_TO_PLANE takes n_i . of both, n_i normalised as the
// functor's constructor does; ROBUST_POINT_TO_POINT applies Ceres' corrector for HuberLoss (rho'' <= 0: residual and Jacobian
// scaled by sqrt(rho')).  Every candidate is evaluated with its Jacobian, so an accepted step needs no second pass.
//
// k_sim3_lm     the group route: one 256-lane workgroup per problem, the whole Levenberg-Marquardt solve in one launch.  Lanes
//               stride over the points; a lane adds its points in ascending index, the wave adds its lanes by the XOR
//               butterfly (wave_reduce.h), and the four wave sums are added in wave order.  Lane 0 holds the state in LDS and
//               runs the 7 x 7 Cholesky and the rules (sim3_advance); the workgroup reads `done` after a barrier, so control
//               flow is uniform.  No atomics: a problem's bytes do not depend on the batch or on the run.
// k_sim3_pass   the grid route, for a problem of more than THEIA_SIM3_GROUP_MAX_POINTS points: workgroup b of a grid that
//               depends on n only owns a fixed contiguous slice of the points and writes its 36 sums to slot b.
// k_sim3_step   one workgroup: lane k adds entry k of the slots in ascending b, lane 0 runs sim3_advance on the state in
//               global memory and leaves the next table T and the `done` flag.  The host enqueues (pass, step) pairs in chunks
//               gated on `done` (device_util.h run_until_done).
// k_sim3_maps   one lane per item for the batched conversions.
#include "sim3_device.h"
#include "lm_rules.h"
#include "wave_reduce.h"
#include "device_util.h"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kSums = 36;      // cost | g [7] | H packed lower [28]
constexpr int kTable = 96;     // sR [9] | t [3] | dsR [9][7] | dt [3][7]
constexpr int kGridSlice = 2048, kGridMaxBlocks = 256;
// what align_point_clouds.cc:258-266 leaves ceres::Solver::Options with (Ceres 2.2)
constexpr double kFunctionTolerance = 1e-6, kGradientTolerance = 1e-10, kParameterTolerance = 1e-8, kMaxRadius = 1e16;

enum { kTypePoint = 0, kTypeRobust = 1, kTypePlane = 2 };

struct Sim3Problem {   // one problem as the kernels see it
  long long first, count;
  double point_weight, huber;
  int type, max_iterations;
};

struct Sim3State {
  double x[7], start[7], cand[7], scale[7], g[7], H[28];
  double cost, initial_cost, gmax, x_norm, model, step_norm;
  double radius, decrease_factor;
  int invalid_steps, step_successful;   // with the two above: the members lm_rules.h works on
  int phase, done, term, pushed, successful, unsuccessful, invalid, rows;
  double alignment_error;
};

// (H + diag(d)) y = g by Cholesky, H packed lower 7 x 7; false on a pivot that is not positive or a non-finite y
__device__ bool solve7(const double* H, const double* d, const double* g, double* y) {
  double L[28];
  for (int a = 0; a < 7; ++a)
    for (int b = 0; b <= a; ++b) {
      double s = H[lm::tri(a, b)] + (a == b ? d[a] : 0.0);
      for (int k = 0; k < b; ++k) s -= L[lm::tri(a, k)] * L[lm::tri(b, k)];
      if (a == b) {
        if (!(s > 0.0)) return false;
        L[lm::tri(a, a)] = sqrt(s);
      } else {
        L[lm::tri(a, b)] = s / L[lm::tri(b, b)];
      }
    }
  double z[7];
  for (int a = 0; a < 7; ++a) {
    double s = g[a];
    for (int k = 0; k < a; ++k) s -= L[lm::tri(a, k)] * z[k];
    z[a] = s / L[lm::tri(a, a)];
  }
  bool finite = true;
  for (int a = 6; a >= 0; --a) {
    double s = z[a];
    for (int k = a + 1; k < 7; ++k) s -= L[lm::tri(k, a)] * y[k];
    y[a] = s / L[lm::tri(a, a)];
    finite = finite && isfinite(y[a]);
  }
  return finite;
}

__device__ void trace_row(double* trace, int capacity_rows, int& rows, double cost, double gmax, double step_norm, double radius,
                          int accepted) {
  if (trace && rows < capacity_rows) {
    double* t = trace + 5 * (size_t)rows;
    t[0] = cost; t[1] = gmax; t[2] = step_norm; t[3] = radius; t[4] = (double)accepted;
  }
  rows += 1;
}

__device__ double norm7(const double* v) {
  double s = 0.0;
  for (int k = 0; k < 7; ++k) s += v[k] * v[k];
  return sqrt(s);
}

__device__ void finish(Sim3State& st, int term, double* T) {
  st.term = term;
  st.done = 1;
  if (term == THEIA_SIM3_TERM_FAILURE)   // Ceres leaves the block of a failed solve as it was passed in
    for (int k = 0; k < 7; ++k) st.x[k] = st.start[k];
  sim3::sim3_exp(st.x, T, T + 9);   // for the alignment error's pass
}

// One thread.  `sums` are the 36 sums of the pass at st.x (phase 0) or at st.cand (phase 1).  Ends with the solve done and T =
// exp(x), or with the next candidate in st.cand and T = exp and its derivative there.
__device__ void sim3_advance(Sim3State& st, const double* sums, int max_iterations, double* T, double* trace, int capacity_rows) {
  if (st.phase == 0) {
    st.cost = 0.5 * sums[0];
    for (int k = 0; k < 7; ++k) st.g[k] = sums[1 + k];
    for (int k = 0; k < 28; ++k) st.H[k] = sums[8 + k];
    for (int k = 0; k < 7; ++k) st.scale[k] = lm::jacobi_scale(st.H[lm::tri(k, k)]);
    st.initial_cost = st.cost;
    st.gmax = 0.0;
    for (int k = 0; k < 7; ++k) st.gmax = fmax(st.gmax, fabs(st.g[k]));
    st.x_norm = norm7(st.x);
    lm::start(st);
    trace_row(trace, capacity_rows, st.rows, st.cost, st.gmax, 0.0, st.radius, 1);
    st.pushed = 1;
    st.phase = 1;
  } else {
    double cand = 0.5 * sums[0];
    if (!isfinite(cand)) cand = DBL_MAX;
    if (lm::parameter_rule(st.step_norm, st.x_norm, kParameterTolerance)) {
      trace_row(trace, capacity_rows, st.rows, cand, st.gmax, st.step_norm, st.radius, 0);
      return finish(st, THEIA_SIM3_TERM_PARAMETER_TOLERANCE, T);
    }
    if (lm::function_rule(st.cost, cand, kFunctionTolerance)) {
      trace_row(trace, capacity_rows, st.rows, cand, st.gmax, st.step_norm, st.radius, 0);
      return finish(st, THEIA_SIM3_TERM_FUNCTION_TOLERANCE, T);
    }
    const double rho = (st.cost - cand) / st.model;
    if (lm::step_accepted(rho)) {
      for (int k = 0; k < 7; ++k) { st.x[k] = st.cand[k]; st.g[k] = sums[1 + k]; }
      for (int k = 0; k < 28; ++k) st.H[k] = sums[8 + k];
      st.x_norm = norm7(st.x);
      st.cost = cand;
      st.gmax = 0.0;
      for (int k = 0; k < 7; ++k) st.gmax = fmax(st.gmax, fabs(st.g[k]));
      lm::accept(st, rho, kMaxRadius);
      st.successful += 1;
      trace_row(trace, capacity_rows, st.rows, st.cost, st.gmax, st.step_norm, st.radius, 1);
    } else {
      lm::shrink(st);
      st.unsuccessful += 1;
      trace_row(trace, capacity_rows, st.rows, cand, st.gmax, st.step_norm, st.radius, 0);
    }
    st.pushed += 1;
  }
  while (true) {
    if (st.pushed - 1 >= max_iterations) return finish(st, THEIA_SIM3_TERM_MAX_ITERATIONS, T);
    if (lm::gradient_rule(st, st.gmax, kGradientTolerance)) return finish(st, THEIA_SIM3_TERM_GRADIENT_TOLERANCE, T);
    if (lm::radius_floor(st)) return finish(st, THEIA_SIM3_TERM_MIN_RADIUS, T);
    double gs[7], Hs[28], d[7], y[7];
    for (int k = 0; k < 7; ++k) gs[k] = st.g[k] * st.scale[k];
    for (int a = 0; a < 7; ++a)
      for (int b = 0; b <= a; ++b) Hs[lm::tri(a, b)] = (st.H[lm::tri(a, b)] * st.scale[a]) * st.scale[b];
    for (int k = 0; k < 7; ++k) d[k] = lm::lm_diagonal(Hs[lm::tri(k, k)], st.radius);
    bool ok = solve7(Hs, d, gs, y);
    double model = 0.0;
    if (ok) {
      model = lm::model_cost_change<7>(Hs, gs, y);
      ok = isfinite(model) && model > 0.0;
    }
    if (!ok) {
      st.invalid += 1;
      if (!lm::invalid_step(st)) return finish(st, THEIA_SIM3_TERM_FAILURE, T);
      trace_row(trace, capacity_rows, st.rows, st.cost, st.gmax, 0.0, st.radius, 0);
      st.pushed += 1;
      continue;
    }
    lm::valid_step(st);
    double delta[7];
    for (int k = 0; k < 7; ++k) { delta[k] = -(y[k] * st.scale[k]); st.cand[k] = st.x[k] + delta[k]; }
    st.step_norm = norm7(delta);
    st.model = model;
    sim3::sim3_exp_d(st.cand, T, T + 9, T + 12, T + 75);
    return;
  }
}

struct Sim3Arrays { const double *source, *target, *weights, *normals; };

// MODE 0: the 36 sums of the points [begin, end) of the problem at the table T; MODE 1: acc[0] = sum |y - (sR x + t)|.
// Lane l takes the points begin + l, begin + l + 256, ... in that order.
template <int MODE>
__device__ __forceinline__ void pass_points(const Sim3Problem& pr, const Sim3Arrays& A, long long begin, long long end,
                                            const double* T, double* acc) {
  for (int k = 0; k < (MODE == 0 ? kSums : 1); ++k) acc[k] = 0.0;
  const double* sR = T;
  const double* t = T + 9;
  const double* dsR = T + 12;
  const double* dt = T + 75;
  const double hub_a = pr.huber, hub_b = pr.huber * pr.huber;
  for (long long i = begin + threadIdx.x; i < end; i += kThreads) {
    const size_t gi = (size_t)(pr.first + i);
    const double x0 = A.source[3 * gi], x1 = A.source[3 * gi + 1], x2 = A.source[3 * gi + 2];
    double d[3];
    for (int r = 0; r < 3; ++r) {
      const double p = ((sR[3 * r] * x0 + sR[3 * r + 1] * x1) + sR[3 * r + 2] * x2) + t[r];
      d[r] = A.target[3 * gi + r] - p;
    }
    if (MODE == 1) {
      acc[0] += sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      continue;
    }
    const double w = A.weights ? A.weights[gi] : pr.point_weight;
    double M[3][7];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 7; ++k)
        M[r][k] = ((dsR[7 * (3 * r) + k] * x0 + dsR[7 * (3 * r + 1) + k] * x1) + dsR[7 * (3 * r + 2) + k] * x2) + dt[7 * r + k];
    if (pr.type == kTypePlane) {
      double n0 = A.normals[3 * gi], n1 = A.normals[3 * gi + 1], n2 = A.normals[3 * gi + 2];
      const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);   // Eigen's normalized()
      n0 /= nn; n1 /= nn; n2 /= nn;
      const double rr = w * ((n0 * d[0] + n1 * d[1]) + n2 * d[2]);
      double J[7];
      for (int k = 0; k < 7; ++k) J[k] = -(w * ((n0 * M[0][k] + n1 * M[1][k]) + n2 * M[2][k]));
      acc[0] += rr * rr;
      for (int k = 0; k < 7; ++k) acc[1 + k] += J[k] * rr;
      for (int a = 0; a < 7; ++a)
        for (int b = 0; b <= a; ++b) acc[8 + lm::tri(a, b)] += J[a] * J[b];
    } else {
      double r[3] = {w * d[0], w * d[1], w * d[2]};
      const double s = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
      double jw = w, rho0 = s;
      if (pr.type == kTypeRobust && s > hub_b) {   // ceres::HuberLoss and the corrector with rho'' <= 0
        const double root = sqrt(s);
        rho0 = 2.0 * hub_a * root - hub_b;
        const double sq = sqrt(fmax(DBL_MIN, hub_a / root));
        r[0] *= sq; r[1] *= sq; r[2] *= sq;
        jw = w * sq;
      }
      acc[0] += rho0;
      for (int r2 = 0; r2 < 3; ++r2)
        for (int k = 0; k < 7; ++k) M[r2][k] = -(jw * M[r2][k]);
      for (int k = 0; k < 7; ++k) acc[1 + k] += (M[0][k] * r[0] + M[1][k] * r[1]) + M[2][k] * r[2];
      for (int a = 0; a < 7; ++a)
        for (int b = 0; b <= a; ++b) acc[8 + lm::tri(a, b)] += (M[0][a] * M[0][b] + M[1][a] * M[1][b]) + M[2][a] * M[2][b];
    }
  }
}

// the workgroup's sums into LDS: the XOR butterfly per wave, then lane k adds entry k of the four wave sums in wave order
template <int N>
__device__ __forceinline__ void team_sums(double* acc, double (*red)[kSums], double* sums /* [N], LDS */) {
  const int wave = threadIdx.x >> 6;
  for (int k = 0; k < N; ++k) acc[k] = wave_sum_butterfly(acc[k]);
  __syncthreads();   // the previous sums' readers are done with red and sums
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < N; ++k) red[wave][k] = acc[k];
  __syncthreads();
  if ((int)threadIdx.x < N) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    sums[threadIdx.x] = s;
  }
  __syncthreads();
}

__device__ void state_begin(Sim3State& st, const double* start) {
  for (int k = 0; k < 7; ++k) { st.x[k] = start[k]; st.start[k] = start[k]; st.cand[k] = start[k]; }
  st.phase = 0; st.done = 0; st.term = 0; st.pushed = 0; st.successful = 0; st.unsuccessful = 0; st.invalid = 0; st.rows = 0;
  st.cost = 0.0; st.initial_cost = 0.0; st.gmax = 0.0; st.x_norm = 0.0; st.model = 0.0; st.step_norm = 0.0;
  st.alignment_error = 0.0;
  lm::start(st);
}

__global__ __launch_bounds__(kThreads) void k_sim3_lm(int count, const int* __restrict__ list, const Sim3Problem* __restrict__ problems,
                                                      Sim3Arrays A, const double* __restrict__ start, double* __restrict__ trace,
                                                      int capacity_rows, Sim3State* __restrict__ out) {
  __shared__ double red[kThreads / 64][kSums];
  __shared__ double T[kTable], sums[kSums];
  __shared__ Sim3State st;
  if ((int)blockIdx.x >= count) return;
  const int p = list[blockIdx.x];
  const Sim3Problem pr = problems[p];
  double* tr = trace ? trace + 5 * (size_t)capacity_rows * p : nullptr;
  if (threadIdx.x == 0) {
    state_begin(st, start + 7 * (size_t)p);
    sim3::sim3_exp_d(st.x, T, T + 9, T + 12, T + 75);
  }
  __syncthreads();
  double acc[kSums];
  while (true) {
    pass_points<0>(pr, A, 0, pr.count, T, acc);
    team_sums<kSums>(acc, red, sums);   // (its barriers also order the readers of T before lane 0 rewrites it)
    if (threadIdx.x == 0) sim3_advance(st, sums, pr.max_iterations, T, tr, capacity_rows);
    __syncthreads();
    if (st.done) break;
  }
  pass_points<1>(pr, A, 0, pr.count, T, acc);
  team_sums<1>(acc, red, sums);
  if (threadIdx.x == 0) {
    st.alignment_error = sums[0] / (double)pr.count;
    out[p] = st;
  }
}

// ---- the grid route
__host__ __device__ inline int grid_blocks(long long n) {
  const long long b = (n + kGridSlice - 1) / kGridSlice;
  return (int)(b < 2 ? 2 : (b > kGridMaxBlocks ? kGridMaxBlocks : b));
}

__global__ __launch_bounds__(kThreads) void k_sim3_begin(const double* __restrict__ start, Sim3State* __restrict__ st,
                                                         double* __restrict__ T) {
  if (threadIdx.x != 0) return;
  state_begin(*st, start);
  sim3::sim3_exp_d(st->x, T, T + 9, T + 12, T + 75);
}

// mode 0: the 36 sums, unless the solve is done; mode 1: the alignment error's sum
__global__ __launch_bounds__(kThreads) void k_sim3_pass(Sim3Problem pr, Sim3Arrays A, const Sim3State* __restrict__ st,
                                                        const double* __restrict__ Tg, double* __restrict__ slots, int mode) {
  __shared__ double red[kThreads / 64][kSums];
  __shared__ double T[kTable], sums[kSums];
  if (mode == 0 && st->done) return;
  if (threadIdx.x < kTable) T[threadIdx.x] = Tg[threadIdx.x];
  __syncthreads();
  const long long B = gridDim.x, slice = (pr.count + B - 1) / B;
  const long long begin = slice * blockIdx.x, end = begin + slice < pr.count ? begin + slice : pr.count;
  double acc[kSums];
  if (mode == 0) {
    pass_points<0>(pr, A, begin, end, T, acc);
    team_sums<kSums>(acc, red, sums);
    if (threadIdx.x < kSums) slots[kSums * (size_t)blockIdx.x + threadIdx.x] = sums[threadIdx.x];
  } else {
    pass_points<1>(pr, A, begin, end, T, acc);
    team_sums<1>(acc, red, sums);
    if (threadIdx.x == 0) slots[kSums * (size_t)blockIdx.x] = sums[0];
  }
}

__global__ __launch_bounds__(kThreads) void k_sim3_step(int blocks, int max_iterations, const double* __restrict__ slots,
                                                        Sim3State* __restrict__ st, double* __restrict__ T,
                                                        double* __restrict__ trace, int capacity_rows) {
  __shared__ double sums[kSums];
  if (st->done) return;
  if (threadIdx.x < kSums) {
    double s = slots[threadIdx.x];
    for (int b = 1; b < blocks; ++b) s += slots[kSums * (size_t)b + threadIdx.x];
    sums[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) sim3_advance(*st, sums, max_iterations, T, trace, capacity_rows);
}

// ---- the conversions
__global__ __launch_bounds__(kThreads) void k_sim3_maps(int op, long long count, const double* __restrict__ in,
                                                        double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  switch (op) {
    case THEIA_SIM3_MAP_EXP: {   // a [7] -> sR [9] | t [3]
      double a[7], o[12];
      for (int k = 0; k < 7; ++k) a[k] = in[7 * i + k];
      sim3::sim3_exp(a, o, o + 9);
      for (int k = 0; k < 12; ++k) out[12 * i + k] = o[k];
    } break;
    case THEIA_SIM3_MAP_LOG: {   // scale | R [9] | t [3] -> a [7]
      double v[13], a[7];
      for (int k = 0; k < 13; ++k) v[k] = in[13 * i + k];
      if (!sim3::sim3_log(v[0], v + 1, v + 10, a))
        for (int k = 0; k < 7; ++k) a[k] = NAN;
      for (int k = 0; k < 7; ++k) out[7 * i + k] = a[k];
    } break;
    case THEIA_SIM3_MAP_FROM_RTS: {   // R [9] | t [3] | scale -> a [7]
      double v[13], a[7];
      for (int k = 0; k < 13; ++k) v[k] = in[13 * i + k];
      if (!sim3::sim3_from_rts(v, v + 9, v[12], a))
        for (int k = 0; k < 7; ++k) a[k] = NAN;
      for (int k = 0; k < 7; ++k) out[7 * i + k] = a[k];
    } break;
    case THEIA_SIM3_MAP_TO_RTS: {   // a [7] -> R [9] | t [3] | scale
      double a[7], o[13];
      for (int k = 0; k < 7; ++k) a[k] = in[7 * i + k];
      sim3::sim3_to_rts(a, o, o + 9, o + 12);
      for (int k = 0; k < 13; ++k) out[13 * i + k] = o[k];
    } break;
    default: {   // THEIA_SIM3_MAP_TO_MATRIX4: a [7] -> [4][4]
      double a[7], o[16];
      for (int k = 0; k < 7; ++k) a[k] = in[7 * i + k];
      sim3::sim3_to_matrix4(a, o);
      for (int k = 0; k < 16; ++k) out[16 * i + k] = o[k];
    } break;
  }
}

int map_widths(int op, int* in_w, int* out_w) {
  switch (op) {
    case THEIA_SIM3_MAP_EXP: *in_w = 7; *out_w = 12; return 0;
    case THEIA_SIM3_MAP_LOG: *in_w = 13; *out_w = 7; return 0;
    case THEIA_SIM3_MAP_FROM_RTS: *in_w = 13; *out_w = 7; return 0;
    case THEIA_SIM3_MAP_TO_RTS: *in_w = 7; *out_w = 13; return 0;
    case THEIA_SIM3_MAP_TO_MATRIX4: *in_w = 7; *out_w = 16; return 0;
  }
  return 1;
}

void fill_summary(const Sim3State& s, int rows_cap, theia_sim3_alignment_summary* o) {
  o->termination = s.term;
  o->success = (s.term == THEIA_SIM3_TERM_GRADIENT_TOLERANCE || s.term == THEIA_SIM3_TERM_FUNCTION_TOLERANCE ||
                s.term == THEIA_SIM3_TERM_PARAMETER_TOLERANCE || s.term == THEIA_SIM3_TERM_MIN_RADIUS) ? 1 : 0;
  o->num_iterations = s.pushed;
  o->num_successful_steps = s.successful;
  o->num_unsuccessful_steps = s.unsuccessful;
  o->num_invalid_steps = s.invalid;
  o->trace_size = std::min(s.rows, rows_cap);
  o->route = 0;
  o->initial_cost = s.initial_cost;
  o->final_cost = s.cost;
  o->alignment_error = s.alignment_error;
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_sim3_maps(int32_t op, int64_t count, const double* in, double* out) {
  int in_w = 0, out_w = 0;
  if (map_widths(op, &in_w, &out_w)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "unknown Sim(3) map %d", (int)op);
  if (count < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative count");
  if (count == 0) return 0;
  if (!in || !out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  int rc = ensure_device();
  if (rc) return rc;
  DevBuf<double> d_in, d_out;
  if ((rc = d_in.up(in, (size_t)in_w * (size_t)count)) || (rc = d_out.alloc((size_t)out_w * (size_t)count))) return rc;
  k_sim3_maps<<<grid_of((size_t)count, kThreads), kThreads>>>(op, (long long)count, d_in.p, d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out.p, sizeof(double) * (size_t)out_w * (size_t)count, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int theia_hip_optimize_alignment_sim3(int32_t num_problems, const int64_t* offsets, const double* source,
                                                 const double* target, const double* weights, const double* normals,
                                                 const double* start, const theia_sim3_alignment_options* options,
                                                 double* params_out, theia_sim3_alignment_summary* summary_out,
                                                 double* trace_out, int32_t trace_capacity, double* timings_ms) {
  const auto t_call = std::chrono::steady_clock::now();
  if (num_problems < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative problem count");
  if (num_problems == 0) {
    if (timings_ms) { timings_ms[0] = 0.0; timings_ms[1] = ms_since(t_call); }
    return 0;
  }
  if (!offsets || !start || !options || !params_out || !summary_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (trace_capacity < 0 || (trace_capacity > 0 && !trace_out)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad trace buffer");
  if (offsets[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  const size_t P = (size_t)num_problems;
  for (size_t p = 0; p < P; ++p)
    if (offsets[p + 1] < offsets[p]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: decreasing offsets", p);
  const size_t total = (size_t)offsets[P];
  if (total > 0 && (!source || !target)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  long long group_max = THEIA_SIM3_GROUP_MAX_POINTS;
  if (const char* e = std::getenv("THEIA_HIP_SIM3_GROUP_MAX_POINTS")) {   // the tests' way to the grid route on a small problem
    const long long v = std::atoll(e);
    if (v >= 1) group_max = v;
  }
  std::vector<Sim3Problem> probs(P);
  std::vector<int> group_list, grid_list;
  for (size_t p = 0; p < P; ++p) {
    const theia_sim3_alignment_options& o = options[p];
    if (o.alignment_type != THEIA_SIM3_POINT_TO_POINT && o.alignment_type != THEIA_SIM3_ROBUST_POINT_TO_POINT &&
        o.alignment_type != THEIA_SIM3_POINT_TO_PLANE)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: unknown alignment type %d", p, (int)o.alignment_type);
    if (o.max_iterations < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: max_iterations < 0", p);
    if (o.alignment_type == THEIA_SIM3_ROBUST_POINT_TO_POINT && !(o.huber_threshold > 0.0 && std::isfinite(o.huber_threshold)))
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: the Huber threshold must be positive", p);
    if (!weights && !std::isfinite(o.point_weight)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: non-finite point_weight", p);
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(start[7 * p + k])) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: non-finite start", p);
    const bool plane = o.alignment_type == THEIA_SIM3_POINT_TO_PLANE && normals;   // without normals: point-to-point (:228-238)
    for (int64_t i = offsets[p]; i < offsets[p + 1]; ++i) {
      for (int k = 0; k < 3; ++k)
        if (!std::isfinite(source[3 * i + k]) || !std::isfinite(target[3 * i + k]))
          return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: non-finite coordinate at point %lld", p, (long long)(i - offsets[p]));
      if (weights && !std::isfinite(weights[i]))
        return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: non-finite weight at point %lld", p, (long long)(i - offsets[p]));
      if (plane) {
        const double* n = normals + 3 * i;
        if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2]))
          return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: non-finite normal at point %lld", p, (long long)(i - offsets[p]));
        if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0)
          return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %zu: zero normal at point %lld", p, (long long)(i - offsets[p]));
      }
    }
    Sim3Problem& q = probs[p];
    q.first = offsets[p]; q.count = offsets[p + 1] - offsets[p];
    q.point_weight = o.point_weight; q.huber = o.huber_threshold; q.max_iterations = o.max_iterations;
    q.type = plane ? kTypePlane : (o.alignment_type == THEIA_SIM3_ROBUST_POINT_TO_POINT ? kTypeRobust : kTypePoint);
    if (q.count == 0) continue;
    (q.count <= group_max ? group_list : grid_list).push_back((int)p);
  }

  int rc = ensure_device();
  if (rc) return rc;
  const int rows_cap = trace_out ? trace_capacity : 0;
  DevBuf<double> d_src, d_tgt, d_w, d_n, d_start, d_trace, d_T, d_slots;
  DevBuf<Sim3Problem> d_probs;
  DevBuf<Sim3State> d_states;
  DevBuf<int> d_list;
  if ((rc = d_src.up(source, 3 * total)) || (rc = d_tgt.up(target, 3 * total)) || (weights && (rc = d_w.up(weights, total))) ||
      (normals && (rc = d_n.up(normals, 3 * total))) || (rc = d_start.up(start, 7 * P)) || (rc = d_probs.up(probs.data(), P)) ||
      (rc = d_states.alloc(P)) || (rc = d_trace.alloc(5 * (size_t)rows_cap * P)) || (rc = d_list.up(group_list.data(), group_list.size())) ||
      (rc = d_T.alloc(kTable)) || (rc = d_slots.alloc((size_t)kSums * kGridMaxBlocks)))
    return rc;
  Sim3Arrays A{d_src.p, d_tgt.p, weights ? d_w.p : nullptr, normals ? d_n.p : nullptr};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (timings_ms) {
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, nullptr));
  }
  if (!group_list.empty())
    k_sim3_lm<<<(unsigned)group_list.size(), kThreads>>>((int)group_list.size(), d_list.p, d_probs.p, A, d_start.p,
                                                         rows_cap ? d_trace.p : nullptr, rows_cap, d_states.p);
  HIP_TRY(hipGetLastError());
  std::vector<Sim3State> h_states(P);
  for (int p : grid_list) {
    const Sim3Problem& q = probs[p];
    const int B = grid_blocks(q.count);
    Sim3State* ds = d_states.p + p;
    double* tr = rows_cap ? d_trace.p + 5 * (size_t)rows_cap * p : nullptr;
    k_sim3_begin<<<1, kThreads>>>(d_start.p + 7 * (size_t)p, ds, d_T.p);
    Sim3State& hs = h_states[p];
    hs.done = 0;
    // every iteration of Ceres' loop takes at most one (pass, step) pair, the start one more
    rc = run_until_done(q.max_iterations + 2, 8, ds, &hs, [&]() {
      k_sim3_pass<<<B, kThreads>>>(q, A, ds, d_T.p, d_slots.p, 0);
      k_sim3_step<<<1, kThreads>>>(B, q.max_iterations, d_slots.p, ds, d_T.p, tr, rows_cap);
      return 0;
    });
    if (rc) return rc;
    if (!hs.done) return set_error(THEIA_HIP_ERR_INTERNAL, "problem %d: the Sim(3) loop did not end", p);
    k_sim3_pass<<<B, kThreads>>>(q, A, ds, d_T.p, d_slots.p, 1);
    HIP_TRY(hipGetLastError());
    std::vector<double> h_slots((size_t)kSums * B);
    HIP_TRY(hipMemcpy(h_slots.data(), d_slots.p, sizeof(double) * h_slots.size(), hipMemcpyDeviceToHost));
    double err = h_slots[0];
    for (int b = 1; b < B; ++b) err += h_slots[(size_t)kSums * b];   // the slots in ascending b
    hs.alignment_error = err / (double)q.count;
  }
  float kernel_ms = 0.f;
  if (timings_ms) {
    hipError_t r = hipEventRecord(e1, nullptr);
    if (r == hipSuccess) r = hipEventSynchronize(e1);
    if (r == hipSuccess) r = hipEventElapsedTime(&kernel_ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIP_TRY(r);
  }
  if (!group_list.empty()) {
    std::vector<Sim3State> all(P);
    HIP_TRY(hipMemcpy(all.data(), d_states.p, sizeof(Sim3State) * P, hipMemcpyDeviceToHost));
    for (int p : group_list) h_states[p] = all[p];
  }
  std::vector<double> h_trace(5 * (size_t)rows_cap * P);
  if (rows_cap) HIP_TRY(hipMemcpy(h_trace.data(), d_trace.p, sizeof(double) * h_trace.size(), hipMemcpyDeviceToHost));
  std::vector<char> is_grid(P, 0);
  for (int p : grid_list) is_grid[p] = 1;
  for (size_t p = 0; p < P; ++p) {
    theia_sim3_alignment_summary& o = summary_out[p];
    if (probs[p].count == 0) {   // "Point clouds cannot be empty." (:172-175): the summary as constructed, the start returned
      o = theia_sim3_alignment_summary{};
      o.termination = THEIA_SIM3_TERM_NO_POINTS;
      for (int k = 0; k < 7; ++k) params_out[7 * p + k] = start[7 * p + k];
      continue;
    }
    fill_summary(h_states[p], rows_cap, &o);
    o.route = is_grid[p];
    for (int k = 0; k < 7; ++k) params_out[7 * p + k] = h_states[p].x[k];
    for (int r = 0; r < o.trace_size; ++r)
      for (int k = 0; k < 5; ++k) trace_out[5 * ((size_t)trace_capacity * p + r) + k] = h_trace[5 * ((size_t)rows_cap * p + r) + k];
  }
  if (timings_ms) { timings_ms[0] = kernel_ms; timings_ms[1] = ms_since(t_call); }
  return 0;
}
