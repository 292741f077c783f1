// ba_covariance.hip -- theia_hip_ba_covariance_full: the camera and point blocks of (J'J)^-1 of a problem in which cameras and
// points are both free (BundleAdjuster::GetCovarianceForTrack(s) / GetCovarianceForView(s), bundle_adjuster.cc:660-773, on
// whatever problem the adjuster holds).  With H = J'J = [U W; W' V], cameras and free intrinsics first, V block diagonal:
//   cov_c = [S^-1]_cc,  S = U - W V^-1 W'  (the reduced camera system at infinite trust radius and unit scales)
//   cov_p = V_p^-1 + V_p^-1 ( sum over observations a, b of p:  W_ap' [S^-1]_ab W_bp ) V_p^-1,   W_ap = F_a' E_a,
// F_a (2 x 6, or 2 x 16 with free intrinsics) the camera side and E_a (2 x d) the point side of observation a's Jacobian.
// S is linearised by the handle's own kernels, copied, repaired at its empty slots and factored once (dense_cholesky.h);
// the needed columns of S^-1 are solved for unit vectors; k_cov_points forms the point blocks, one wavefront per track.
#include <cmath>
#include <cstdio>

#include "ba_handle.h"

namespace thip {
namespace {

// A point block's pivot counts as not positive when it is rounding noise of its diagonal entry: the last pivot of a track
// with one observation (V_p = E'E of rank 2) or of an un-parametrised homogeneous point (d = 4, rank 3) is a difference of
// equal numbers, of either sign.
constexpr double kCovPivotTol = 1e-13;
constexpr int kCovTile = 16;            // observations per LDS tile of k_cov_points
constexpr int kCovDefaultChunk = 1024;  // unit vectors per solve when the caller leaves max_rhs_columns to the library

double g_cov_phase_ms[4] = {0.0, 0.0, 0.0, 0.0};   // linearise + copy, factorisation, column solves, block kernels of the last call

// first / one-past-last sorted observation of every point that has non-fixed observations (both arrays zeroed before)
__global__ void k_cov_track_ranges(int64_t nm, const int* __restrict__ obs_pt, int* __restrict__ trk_start, int* __restrict__ trk_end) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= nm) return;
  const int p = obs_pt[o];
  if (o == 0 || obs_pt[o - 1] != p) trk_start[p] = (int)o;
  if (o == nm - 1 || obs_pt[o + 1] != p) trk_end[p] = (int)o + 1;
}

// live[i]: slot i of the reduced system is a free parameter whose row is not empty
__global__ void k_cov_live(int n, const uint8_t* __restrict__ free_slot, const double* __restrict__ S, uint8_t* __restrict__ live) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) live[i] = (free_slot[i] && S[(size_t)i * n + i] != 0.0) ? 1 : 0;
}

// The lower triangle of S into the system that is factored (leading dimension lda, cleared before); the slots that are not
// live -- frozen intrinsics, masked camera columns, unobserved blocks -- get a unit diagonal and nothing else.
__global__ void k_cov_copy_repair(int n, const double* __restrict__ S, const uint8_t* __restrict__ live, double* __restrict__ A, int lda) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)n * n) return;
  const int i = (int)(e / n), j = (int)(e - (size_t)i * n);
  if (j > i) return;
  A[(size_t)i * lda + j] = (live[i] && live[j]) ? S[e] : (i == j ? 1.0 : 0.0);
}

// need[slot] = 1 for the reduced columns of every camera and intrinsics group a selected track is seen by
__global__ void k_cov_mark_needed(int nsel, const int* __restrict__ sel, const int* __restrict__ trk_start, const int* __restrict__ trk_end,
                                  const int* __restrict__ obs_cam, const int* __restrict__ cam_red, const int* __restrict__ cam_group,
                                  const int* __restrict__ grp_red, int ni, uint8_t* __restrict__ need) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsel) return;
  const int p = sel[s];
  for (int o = trk_start[p]; o < trk_end[p]; ++o) {
    const int c = obs_cam[o], rc = cam_red[c];
    if (rc >= 0) for (int q = 0; q < 6; ++q) need[ni + 6 * rc + q] = 1;
    if (ni) {
      const int gr = grp_red[cam_group[c]];
      if (gr >= 0) for (int q = 0; q < 10; ++q) need[10 * gr + q] = 1;
    }
  }
}

// B [k][n] (cleared before): row j = the unit vector of column cols[j]
__global__ void k_cov_unit(int k, int n, const int* __restrict__ cols, double* __restrict__ B) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < k) B[(size_t)j * n + cols[j]] = 1.0;
}

// One lane group per selected camera gathers its 6 x 6 from X [k][n] (row xrow[s] = S^-1 e_s); rows and columns of frozen
// parameters stay zero.  Entry (a, b) is read from the row of the smaller slot: the block is symmetric bit for bit.
__global__ __launch_bounds__(64) void k_cov_cam_blocks(int nsel, const int* __restrict__ sel_cam, const int* __restrict__ cam_red, int ni,
                                                       int n, const uint8_t* __restrict__ live, const int* __restrict__ xrow,
                                                       const double* __restrict__ X, double* __restrict__ out) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= nsel || lane >= 36) return;
  const int rc = cam_red[sel_cam[s]];
  const int a = lane / 6, b = lane - 6 * a;
  const int lo = ni + 6 * rc + min(a, b), hi = ni + 6 * rc + max(a, b);
  double v = 0.0;
  if (live[lo] && live[hi] && xrow[lo] >= 0) v = X[(size_t)xrow[lo] * n + hi];
  out[(size_t)s * 36 + lane] = v;
}

struct CovPointsArgs {
  int n, ni, nsel;
  const int* sel;          // [nsel] point indices (variable points)
  const int* trk_start;    // [np] sorted-observation range of a point
  const int* trk_end;
  const int* obs_cam;      // [nobs] sorted
  const int* cam_red; const int* cam_group; const int* grp_red;
  const uint8_t* live;     // [n]
  const int* xrow;         // [n] row of X that holds S^-1 e_slot, -1 = not solved
  const double* X;         // [k][n]
  const double* jc;        // [nobs_main][2][6]  camera side (launch_evaluate: loss-corrected, masked, unscaled)
  const double* jp;        // [nobs_main][2][PD] point side, tangent space
  const double* ji;        // [nobs_main][2][10] intrinsics side (INTR)
  double* out;             // [nsel][PD][PD]
  int* fail;               // max over the tracks with a pivot that is not positive of (point index + 1)
};

template <int N>
__device__ __forceinline__ void wave_sum_all_fixed(double (&v)[N]) {   // xor butterfly: every lane ends with the same bits
#pragma unroll
  for (int f = 0; f < N; ++f)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[f] += __shfl_xor(v[f], off, 64);
}

// The hot kernel: one wavefront per selected track.  Y_a = W_a V_p^-1 has rank two, Y_a = F_a' G_a with G_a = E_a V_p^-1
// (2 x d), so a pair's term Y_a' Z_ab Y_b is G_a' (F_a Z_ab F_b') G_b: the lane that owns the pair (a, b), b <= a, gathers
// Z_ab = [S^-1] at (columns of a, columns of b) through the two observations' reduced column lists into a 2 x 2 and adds
// the term and its transpose (the pair (b, a)).  F, G and the column lists of kCovTile observations at a time sit in LDS; a
// longer track walks its pair tiles (ta, tb <= ta) in order.  Every lane sums its pairs in index order and the lanes are
// summed by a butterfly: no atomics, the same bytes on every run for the same X and Jacobians.
template <int PD, bool INTR>
__global__ __launch_bounds__(64) void k_cov_points(CovPointsArgs A) {
  constexpr int NC = INTR ? 16 : 6, T = kCovTile, NT = PD * (PD + 1) / 2, O = INTR ? 10 : 0;
  __shared__ double sF[2][T][2 * NC + 1];
  __shared__ double sG[2][T][2 * PD + 1];
  __shared__ int sC[2][T][NC + 1];   // reduced column of the observation's camera-side column, -1 = not a live parameter
  __shared__ int sR[2][T][NC + 1];   // its row in X
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  if (s >= A.nsel) return;
  const int p = A.sel[s];
  const int o0 = A.trk_start[p], m = A.trk_end[p] - o0;
  double* out = A.out + (size_t)s * PD * PD;
  if (m <= 0) {   // unobserved: a zero block
    if (lane < PD * PD) out[lane] = 0.0;
    return;
  }
  // V_p = sum E_a' E_a (lower triangle), the same on every lane
  double v[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) v[i] = 0.0;
  for (int a = lane; a < m; a += 64) {
    const double* J = A.jp + (size_t)2 * PD * (o0 + a);
#pragma unroll
    for (int r = 0; r < PD; ++r)
#pragma unroll
      for (int c = 0; c <= r; ++c) v[r * (r + 1) / 2 + c] += J[r] * J[c] + J[PD + r] * J[PD + c];
  }
  wave_sum_all_fixed<NT>(v);
  // V_p^-1 by Cholesky: V = L L', Li = L^-1, V^-1 = Li' Li
  double L[PD][PD], Li[PD][PD], Vi[PD][PD];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < PD; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double t = v[i * (i + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(t > kCovPivotTol * v[i * (i + 1) / 2 + i])) ok = false;
        L[i][i] = sqrt(t);
      } else L[i][j] = t / L[j][j];
    }
  if (!ok) {   // (uniform: every lane holds the same V)
    if (lane == 0) atomicMax(A.fail, p + 1);
    if (lane < PD * PD) out[lane] = 0.0;
    return;
  }
#pragma unroll
  for (int i = 0; i < PD; ++i) {
#pragma unroll
    for (int j = 0; j < PD; ++j) Li[i][j] = 0.0;
    Li[i][i] = 1.0 / L[i][i];
#pragma unroll
    for (int j = 0; j < i; ++j) {
      double t = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) t -= L[i][k] * Li[k][j];
      Li[i][j] = t / L[i][i];
    }
  }
#pragma unroll
  for (int a = 0; a < PD; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      double t = 0.0;
#pragma unroll
      for (int k = a; k < PD; ++k) t += Li[k][a] * Li[k][b];
      Vi[a][b] = t; Vi[b][a] = t;
    }

  auto load_tile = [&](int buf, int t) {
    const int a = t * T + lane;
    if (lane < T && a < m) {
      const size_t o = (size_t)o0 + a;
      const int c = A.obs_cam[o], rc = A.cam_red[c];
      double* F = sF[buf][lane];
      int* C = sC[buf][lane];
      int* R = sR[buf][lane];
      if constexpr (INTR) {
        const int gr = A.grp_red[A.cam_group[c]];
        const double* K = A.ji + 20 * o;
        for (int q = 0; q < 10; ++q) {
          F[q] = K[q]; F[NC + q] = K[10 + q];
          int col = gr >= 0 ? 10 * gr + q : -1;
          if (col >= 0 && !A.live[col]) col = -1;
          C[q] = col; R[q] = col >= 0 ? A.xrow[col] : -1;
        }
      }
      const double* E = A.jc + 12 * o;
      for (int q = 0; q < 6; ++q) {
        F[O + q] = E[q]; F[NC + O + q] = E[6 + q];
        int col = rc >= 0 ? A.ni + 6 * rc + q : -1;
        if (col >= 0 && !A.live[col]) col = -1;
        C[O + q] = col; R[O + q] = col >= 0 ? A.xrow[col] : -1;
      }
      const double* J = A.jp + 2 * PD * o;
      double* G = sG[buf][lane];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < PD; ++r) {
          double t = 0.0;
#pragma unroll
          for (int q = 0; q < PD; ++q) t += J[u * PD + q] * Vi[q][r];
          G[u * PD + r] = t;
        }
    }
  };

  double acc[PD * PD];
#pragma unroll
  for (int i = 0; i < PD * PD; ++i) acc[i] = 0.0;
  const int nt = (m + T - 1) / T;
  for (int ta = 0; ta < nt; ++ta) {
    __syncthreads();
    load_tile(0, ta);
    const int na = min(T, m - ta * T);
    for (int tb = 0; tb <= ta; ++tb) {
      const int sb = tb == ta ? 0 : 1;
      if (sb) { __syncthreads(); load_tile(1, tb); }
      __syncthreads();
      const int nb = min(T, m - tb * T);
      for (int idx = lane; idx < na * nb; idx += 64) {
        const int a = idx / nb, b = idx - a * nb;
        if (!sb && b > a) continue;
        const double* Fa = sF[0][a];
        const double* Fb = sF[sb][b];
        const int* Ca = sC[0][a];
        const int* Rb = sR[sb][b];
        double k00 = 0.0, k01 = 0.0, k10 = 0.0, k11 = 0.0;   // F_a Z_ab F_b'
        for (int j = 0; j < NC; ++j) {
          const int rj = Rb[j];
          if (rj < 0) continue;
          const double* Xr = A.X + (size_t)rj * A.n;   // S^-1 e_(column j of b): entry (column i of a) is Z_ab[i][j]
          double t0 = 0.0, t1 = 0.0;
          for (int i = 0; i < NC; ++i) {
            const int ci = Ca[i];
            if (ci < 0) continue;
            const double z = Xr[ci];
            t0 += Fa[i] * z; t1 += Fa[NC + i] * z;
          }
          k00 += t0 * Fb[j]; k01 += t0 * Fb[NC + j];
          k10 += t1 * Fb[j]; k11 += t1 * Fb[NC + j];
        }
        const double* Ga = sG[0][a];
        const double* Gb = sG[sb][b];
        double h0[PD], h1[PD], gb0[PD], gb1[PD];
#pragma unroll
        for (int r = 0; r < PD; ++r) {
          h0[r] = Ga[r] * k00 + Ga[PD + r] * k10;
          h1[r] = Ga[r] * k01 + Ga[PD + r] * k11;
          gb0[r] = Gb[r]; gb1[r] = Gb[PD + r];
        }
        const bool diag = !sb && a == b;
#pragma unroll
        for (int r = 0; r < PD; ++r)
#pragma unroll
          for (int c = 0; c < PD; ++c) {
            const double mrc = h0[r] * gb0[c] + h1[r] * gb1[c];
            const double mcr = h0[c] * gb0[r] + h1[c] * gb1[r];
            acc[r * PD + c] += diag ? mrc : mrc + mcr;
          }
      }
    }
  }
  wave_sum_all_fixed<PD * PD>(acc);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < PD; ++r)
#pragma unroll
      for (int c = 0; c < PD; ++c) out[r * PD + c] = Vi[r][c] + 0.5 * (acc[r * PD + c] + acc[c * PD + r]);
  }
}

void launch_cov_points(const CovPointsArgs& A, int pd, bool intr, hipStream_t st) {
  if (A.nsel <= 0) return;
  if (pd == 3) {
    if (intr) k_cov_points<3, true><<<A.nsel, 64, 0, st>>>(A);
    else k_cov_points<3, false><<<A.nsel, 64, 0, st>>>(A);
  } else {
    if (intr) k_cov_points<4, true><<<A.nsel, 64, 0, st>>>(A);
    else k_cov_points<4, false><<<A.nsel, 64, 0, st>>>(A);
  }
}

struct CovEvents {   // phase boundaries on the handle's stream
  hipEvent_t e[5] = {};
  int made = 0;
  int create() {
    for (; made < 5; ++made) HIP_TRYR(hipEventCreate(&e[made]));
    return 0;
  }
  ~CovEvents() { for (int i = 0; i < made; ++i) (void)hipEventDestroy(e[i]); }
};

}  // namespace
}  // namespace thip

extern "C" {

int theia_hip_ba_covariance_full(theia_ba_handle h, int32_t num_view_sel, const int32_t* view_sel, int32_t num_track_sel,
                                 const int32_t* track_sel, int32_t max_rhs_columns, double* cam_cov, double* point_cov) {
  if (h && h->idh) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "inverse-depth handle: covariance is not built in this mode");
  if (!h) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle");
  if (h->shard_world > 1 || h->allreduce)
    return set_error(THEIA_HIP_ERR_UNSUPPORTED, "covariance of a sharded handle: the reduced system of one rank is a partial sum");
  if (num_view_sel < 0 || num_track_sel < 0 || max_rhs_columns < 0 || (num_view_sel > 0 && !view_sel) || (num_track_sel > 0 && !track_sel))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad selection");
  for (int i = 0; view_sel && i < num_view_sel; ++i)
    if (view_sel[i] < 0 || view_sel[i] >= h->nc) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view_sel[%d] = %d is not a camera", i, view_sel[i]);
  for (int i = 0; track_sel && i < num_track_sel; ++i)
    if (track_sel[i] < 0 || track_sel[i] >= h->np) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track_sel[%d] = %d is not a point", i, track_sel[i]);
  release_stage_if_idle(h);
  if (!cam_cov && !point_cov) return 0;
  const int pd = h->pd, n = h->n, ni = h->ni;
  hipStream_t st = h->stream;
  int rc;

  // the selected blocks that exist: variable cameras, variable points
  std::vector<int> sel_cam, sel_pt;
  if (cam_cov) {
    std::fill(cam_cov, cam_cov + 36 * (size_t)h->nc, 0.0);
    const int cnt = view_sel ? num_view_sel : h->nc;
    for (int i = 0; i < cnt; ++i) { const int c = view_sel ? view_sel[i] : i; if (h->cam_red[c] >= 0) sel_cam.push_back(c); }
  }
  if (point_cov) {
    std::fill(point_cov, point_cov + (size_t)pd * pd * h->np, 0.0);
    const int cnt = track_sel ? num_track_sel : h->np;
    for (int i = 0; i < cnt; ++i) { const int q = track_sel ? track_sel[i] : i; if (!h->pt_const[q]) sel_pt.push_back(q); }
  }
  if (sel_cam.empty() && sel_pt.empty()) return 0;

  // which slots of the reduced system are parameters at all
  std::vector<uint8_t> free_slot((size_t)std::max(1, n), 0);
  for (int g = 0; g < (int)h->grp_red.size(); ++g) {
    const int gr = h->grp_red[g];
    if (gr < 0 || !ni) continue;
    for (int q = 0; q < 10; ++q) free_slot[10 * gr + q] = (q < h->grp_k[g] && ((h->grp_free[g] >> q) & 1u)) ? 1 : 0;
  }
  for (int c = 0; c < h->nc; ++c) {
    const int r = h->cam_red[c];
    if (r < 0) continue;
    for (int q = 0; q < 6; ++q) free_slot[ni + 6 * r + q] = ((h->cam_mask[c] >> q) & 1u) ? 0 : 1;
  }

  CovEvents ev;
  if ((rc = ev.create())) return rc;
  DenseSpd sys;
  PoolBuf<uint8_t> d_free, d_live, d_need;
  PoolBuf<int> d_trk, d_sel_pt, d_sel_cam, d_cols, d_xrow, d_fail;
  PoolBuf<double> d_jc, d_jp, d_ji, d_X, d_B, d_T, d_pout, d_cout;
  // (declared behind the buffers: on every way out the stream is drained before a block goes back to the device cache)
  struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};
  const size_t nm = (size_t)h->nobs_main;
  if ((rc = sys.alloc(n, 1)) || (rc = d_free.upload(free_slot, st)) || (rc = d_live.alloc((size_t)std::max(1, n))) ||
      (rc = d_need.alloc((size_t)std::max(1, n))) || (rc = d_fail.alloc(1)))
    return rc;
  HIP_TRYR(hipMemsetAsync(d_fail.p, 0, sizeof(int), st));

  // ---- linearise at the current state: unit scales, no damping (as theia_hip_ba_covariance), camera priors included
  HIP_TRYR(hipEventRecord(ev.e[0], st));
  DevProblem Q = h->P;
  Q.scale_c = h->ones_c.p; Q.scale_p = h->ones_p.p; Q.scale_i = h->ones_i.p; Q.intr = h->intr[h->cur].p;
  Q.camrot_current = 0; h->camrot_valid = false;   // (the per-camera blocks are rebuilt with the unit scales, and are the solve's no longer)
  LmState lm;
  std::memset(&lm, 0, sizeof(lm));
  lm.radius = 1e300;
  HIP_TRYR(hipMemcpyAsync(h->lm_state.p, &lm, sizeof(lm), hipMemcpyHostToDevice, st));
  HIP_TRYR(hipStreamSynchronize(st));   // `lm` is a stack object
  const double* radius = &reinterpret_cast<const LmState*>(h->lm_state.p)->radius;
  if (n > 0) {
    HIP_TRYR(hipMemsetAsync(h->reduce.p, 0, sizeof(double) * h->reduce.n, st));
    if (h->Vinv.n) HIP_TRYR(hipMemsetAsync(h->Vinv.p, 0, sizeof(double) * h->Vinv.n, st));
    launch_linearize(Q, h->cam[h->cur].p, h->pts[h->cur].p, radius, h->rb, h->Vinv.p, h->gp.p, h->tile_part.p, st);
    launch_long_linearize(Q, h->cam[h->cur].p, h->pts[h->cur].p, radius, h->rb, h->Vinv.p, h->gp.p, h->long_scratch.p, st);
    launch_cam_priors(Q, PRIOR_LINEARIZE, h->cam[h->cur].p, nullptr, nullptr, &h->rb, nullptr, h->rb.scal + SC_COST, nullptr, st);
    // ---- a system of its own: copy, repair the empty slots, factor once
    if ((rc = sys.clear(st, true))) return rc;
    k_cov_live<<<grid_of((size_t)n, 256), 256, 0, st>>>(n, d_free.p, h->rb.S, d_live.p);
    k_cov_copy_repair<<<grid_of((size_t)n * n, 256), 256, 0, st>>>(n, h->rb.S, d_live.p, sys.A(), sys.lda);
  }
  // ---- the tracks' observation ranges and Jacobians (launch_evaluate: sorted order, tangent space, loss applied)
  if (!sel_pt.empty()) {
    if ((rc = d_trk.alloc(2 * (size_t)h->np)) || (rc = d_sel_pt.upload(sel_pt, st)) || (rc = d_jc.alloc(12 * nm)) ||
        (rc = d_jp.alloc(2 * (size_t)pd * nm)) || (ni && (rc = d_ji.alloc(20 * nm))) || (rc = d_pout.alloc((size_t)pd * pd * sel_pt.size())))
      return rc;
    HIP_TRYR(hipMemsetAsync(d_trk.p, 0, sizeof(int) * 2 * (size_t)h->np, st));
    if (nm) k_cov_track_ranges<<<grid_of(nm, 256), 256, 0, st>>>((int64_t)nm, h->obs_pt.p, d_trk.p, d_trk.p + h->np);
    DevProblem E = Q;
    E.ntiles = h->ntiles_eval;
    launch_evaluate(E, h->cam[h->cur].p, h->pts[h->cur].p, nullptr, d_jc.p, d_jp.p, nullptr, h->tile_part.p, st, ni ? d_ji.p : nullptr);
  }
  HIP_TRYR(hipEventRecord(ev.e[1], st));
  if (n > 0) sys.factor(1, st);
  HIP_TRYR(hipEventRecord(ev.e[2], st));

  // ---- the columns of S^-1 that are needed
  std::vector<uint8_t> live((size_t)std::max(1, n), 0), need((size_t)std::max(1, n), 0);
  std::vector<int> cols, xrow((size_t)std::max(1, n), -1);
  if (n > 0) {
    const bool all_points = point_cov && !track_sel;
    if (!all_points) {
      HIP_TRYR(hipMemsetAsync(d_need.p, 0, (size_t)n, st));
      if (!sel_pt.empty())
        k_cov_mark_needed<<<grid_of(sel_pt.size(), 256), 256, 0, st>>>((int)sel_pt.size(), d_sel_pt.p, d_trk.p, d_trk.p + h->np, h->obs_cam.p,
                                                                       h->d_cam_red.p, h->cam_group.p, h->d_grp_red.p, ni, d_need.p);
      HIP_TRYR(hipMemcpyAsync(need.data(), d_need.p, (size_t)n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRYR(hipMemcpyAsync(live.data(), d_live.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRYR(hipStreamSynchronize(st));
    bool failed = false;
    if ((rc = sys.failed(&failed))) return rc;
    if (failed) { release_stage_if_idle(h); return set_error(THEIA_HIP_ERR_INTERNAL, "reduced camera system: J'J is rank deficient (ceres::Covariance::Compute fails)"); }
    if (all_points) std::fill(need.begin(), need.end(), (uint8_t)1);
    for (int c : sel_cam) for (int q = 0; q < 6; ++q) need[ni + 6 * h->cam_red[c] + q] = 1;
    for (int i = 0; i < n; ++i) if (need[i] && live[i]) { xrow[i] = (int)cols.size(); cols.push_back(i); }
  }
  const int k = (int)cols.size();
  const int chunk = std::max(1, std::min(std::min(k, 65535), max_rhs_columns > 0 ? (int)max_rhs_columns : kCovDefaultChunk));
  if (k > 0) {
    if ((rc = d_X.alloc((size_t)k * n)) || (rc = d_B.alloc((size_t)chunk * n)) || (rc = d_T.alloc((size_t)chunk * n)) || (rc = d_cols.upload(cols, st)))
      return rc;
  }
  if ((rc = d_xrow.upload(xrow, st))) return rc;
  for (int c0 = 0; c0 < k; c0 += chunk) {
    const int kc = std::min(chunk, k - c0);
    HIP_TRYR(hipMemsetAsync(d_B.p, 0, sizeof(double) * (size_t)kc * n, st));
    k_cov_unit<<<grid_of((size_t)kc, 256), 256, 0, st>>>(kc, n, d_cols.p + c0, d_B.p);
    dense_cholesky_solve_factored(n, sys.A(), sys.lda, sys.work.p, kc, d_B.p, n, d_T.p, d_X.p + (size_t)c0 * n, n, st);
  }
  HIP_TRYR(hipEventRecord(ev.e[3], st));

  // ---- the blocks
  std::vector<double> cout_h, pout_h;
  if (!sel_cam.empty()) {
    if ((rc = d_sel_cam.upload(sel_cam, st)) || (rc = d_cout.alloc(36 * sel_cam.size()))) return rc;
    k_cov_cam_blocks<<<(int)sel_cam.size(), 64, 0, st>>>((int)sel_cam.size(), d_sel_cam.p, h->d_cam_red.p, ni, n, d_live.p, d_xrow.p, d_X.p, d_cout.p);
    cout_h.resize(36 * sel_cam.size());
    HIP_TRYR(hipMemcpyAsync(cout_h.data(), d_cout.p, sizeof(double) * cout_h.size(), hipMemcpyDeviceToHost, st));
  }
  if (!sel_pt.empty()) {
    CovPointsArgs A;
    A.n = n; A.ni = ni; A.nsel = (int)sel_pt.size();
    A.sel = d_sel_pt.p; A.trk_start = d_trk.p; A.trk_end = d_trk.p + h->np;
    A.obs_cam = h->obs_cam.p; A.cam_red = h->d_cam_red.p; A.cam_group = h->cam_group.p; A.grp_red = h->d_grp_red.p;
    A.live = d_live.p; A.xrow = d_xrow.p; A.X = d_X.p;
    A.jc = d_jc.p; A.jp = d_jp.p; A.ji = d_ji.p;
    A.out = d_pout.p; A.fail = d_fail.p;
    launch_cov_points(A, pd, ni != 0, st);
    pout_h.resize((size_t)pd * pd * sel_pt.size());
    HIP_TRYR(hipMemcpyAsync(pout_h.data(), d_pout.p, sizeof(double) * pout_h.size(), hipMemcpyDeviceToHost, st));
  }
  HIP_TRYR(hipEventRecord(ev.e[4], st));
  int fail = 0;
  HIP_TRYR(hipMemcpyAsync(&fail, d_fail.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  for (int i = 0; i < 4; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
    g_cov_phase_ms[i] = ms;
  }
  release_stage_if_idle(h);
  if (fail) {
    if (point_cov) std::fill(point_cov, point_cov + (size_t)pd * pd * h->np, 0.0);
    return set_error(THEIA_HIP_ERR_INTERNAL, "point %d: J'J is rank deficient (ceres::Covariance::Compute fails)", fail - 1);
  }
  for (size_t i = 0; i < sel_cam.size(); ++i) std::copy(&cout_h[36 * i], &cout_h[36 * i] + 36, cam_cov + 36 * (size_t)sel_cam[i]);
  for (size_t i = 0; i < sel_pt.size(); ++i)
    std::copy(&pout_h[(size_t)pd * pd * i], &pout_h[(size_t)pd * pd * i] + pd * pd, point_cov + (size_t)pd * pd * sel_pt[i]);
  return 0;
}

int theia_hip_ba_free_parameter_count(theia_ba_handle h, int64_t* count) {
  if (h && h->idh) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "inverse-depth handle: the parameter count is not built in this mode");
  if (!h || !count) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  int64_t c = 0;
  for (int i = 0; i < h->nc; ++i) if (h->cam_red[i] >= 0) c += 6 - __builtin_popcount(h->cam_mask[i] & 0x3fu);
  if (h->ni)
    for (int g = 0; g < (int)h->grp_red.size(); ++g)
      if (h->grp_red[g] >= 0) c += __builtin_popcount(h->grp_free[g] & ((1u << h->grp_k[g]) - 1u));
  for (int q = 0; q < h->np; ++q) if (!h->pt_const[q]) c += h->pd;
  *count = c;
  return 0;
}

int theia_hip_ba_covariance_full_timing(double* phase_ms) {
  if (!phase_ms) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  for (int i = 0; i < 4; ++i) phase_ms[i] = g_cov_phase_ms[i];
  return 0;
}

}  // extern "C"
