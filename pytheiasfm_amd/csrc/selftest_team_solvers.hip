// selftest_team_solvers.hip -- test-only entry points for the team linear algebra of the minimal solvers: the eigen-solver
// teams (eig_team.h), the 9 x 9 SVD teams (svd_team.h) and stage A of the five-point solver (fit5_team.h), each run next to
// the one-thread routine it claims to be bit-identical to (eig_general.h: eig_general_t, small_linalg.h: svd_sq<9>, five_point_device.h: five_point_pre) on
// matrices the caller chooses.  The team kernels keep the production launch shapes: 64-lane blocks, the callers' teams per
// wave (idle lanes included) and their LDS layouts; a team whose matrix is masked off returns at once, as the production
// teams of a hypothesis past active_iters do.  Nothing here runs on the estimation path.
#include "ransac_device.h"
#include "eig_team.h"
#include "svd_team.h"
#include "fit5_team.h"
#include "dls_device.h"
#include "device_util.h"

#include <algorithm>
#include <vector>

namespace thip {
namespace {

// ---- eigen-decomposition.  Record per matrix (doubles): ok | wr [n] | wi [n] | H [n][n] (the Schur form) | V [n][n]
// (the kept rows only, NR x n, when NR > 0).
__host__ __device__ inline size_t eig_record(int n) { return 1 + 2 * (size_t)n + 2 * (size_t)n * n; }

// XMODE 0: X in LDS after V (k_upnp_b, k_p4pfr_b: H | V | X | wr | wi | ort at n x n strides).
// XMODE 1: X = the matrix's own global slot, H | V | wr | wi | ort at MAXN strides (k_fit5_b).
// XMODE 2: V = X = the matrix's own global slot, H | kept rows | wr | wi | ort at MAXN strides (k_dls_b_team, k_gdls_b_team).
template <int TEAM, bool CPLX, int NR, int MAXN, int XMODE>
__global__ __launch_bounds__(64) void k_selftest_eig_team(int n, int count, const int* __restrict__ active, double* work,
                                                          double* __restrict__ out) {
  constexpr int kTeamsPerWave = 64 / TEAM;
  constexpr int kLds = XMODE == 0 ? 3 * MAXN * MAXN + 3 * MAXN
                     : XMODE == 1 ? 2 * MAXN * MAXN + 3 * MAXN
                                  : MAXN * MAXN + NR * MAXN + 3 * MAXN;
  __shared__ double lds[kTeamsPerWave][kLds];
  const int team = threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
  const int i = blockIdx.x * kTeamsPerWave + team;
  if (team >= kTeamsPerWave || i >= count || !active[i]) return;
  const int s2 = XMODE == 0 ? n * n : MAXN * MAXN, s1 = XMODE == 0 ? n : MAXN;
  double* H = lds[team];
  double* V = H + s2;    // (XMODE 2: the kept rows Vk)
  double* X = XMODE == 0 ? V + s2 : nullptr;
  double* wr = XMODE == 0 ? X + s2 : (XMODE == 1 ? V + s2 : V + NR * s1);
  double* wi = wr + s1;
  double* ort = wi + s1;
  double* w = work + (size_t)i * n * n;
  for (int e = tl; e < n * n; e += TEAM) H[e] = w[e];
  rsc::team_sync();
  bool good;
  if constexpr (XMODE == 2) good = rsc::eig_team<TEAM, true, NR>(n, H, w, w, wr, wi, ort, tl, V, dlsdev::kKeptRow);
  else good = rsc::eig_team<TEAM, CPLX>(n, H, V, XMODE == 0 ? X : w, wr, wi, ort, tl);
  rsc::team_sync();
  double* o = out + (size_t)i * eig_record(n);
  if (tl == 0) o[0] = good ? 1.0 : 0.0;
  for (int e = tl; e < n; e += TEAM) { o[1 + e] = wr[e]; o[1 + n + e] = wi[e]; }
  for (int e = tl; e < n * n; e += TEAM) o[1 + 2 * n + e] = H[e];
  const int vrows = NR > 0 ? NR : n;
  for (int e = tl; e < vrows * n; e += TEAM) o[1 + 2 * n + n * n + e] = V[e];
}

// one thread per matrix: eig_general_t without V (its H is then the Schur form) and with V (the eigenvalues and vectors).
// The two runs take the same decisions; a record whose eigenvalues differ between them gets ok = -1.
template <int MAXN, bool CPLX>
__global__ __launch_bounds__(64) void k_selftest_eig_single(int n, int count, const int* __restrict__ active,
                                                            const double* __restrict__ A, double* __restrict__ work,
                                                            double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count || !active[i]) return;
  const double* a = A + (size_t)i * n * n;
  double* w = work + (size_t)i * n * n;
  double* o = out + (size_t)i * eig_record(n);
  double* Hs = o + 1 + 2 * n;
  for (int e = 0; e < n * n; ++e) { Hs[e] = a[e]; w[e] = a[e]; }
  double wr[MAXN], wi[MAXN];
  const bool ok_schur = rsc::eig_general_t<MAXN, CPLX>(n, Hs, wr, wi, nullptr);
  const bool ok = rsc::eig_general_t<MAXN, CPLX>(n, w, o + 1, o + 1 + n, o + 1 + 2 * n + n * n);
  bool same = ok == ok_schur;
  if (ok && ok_schur)
    for (int e = 0; e < n; ++e)
      same = same && __double_as_longlong(wr[e]) == __double_as_longlong(o[1 + e]) &&
             __double_as_longlong(wi[e]) == __double_as_longlong(o[1 + n + e]);
  o[0] = same ? (ok ? 1.0 : 0.0) : -1.0;
}

// ---- 9 x 9 SVD.  Record per matrix: U [81] | S [9] | V [81] (V untouched by a team run without V).
constexpr int kSvdRecord = 171;
template <int TEAM, bool WITH_V>
__global__ __launch_bounds__(64) void k_selftest_svd9_team(int count, const double* __restrict__ A, double* __restrict__ out) {
  constexpr int kTeamsPerWave = 64 / TEAM;
  __shared__ double lds[kTeamsPerWave][81 + 81 + (WITH_V ? 81 : 0) + 9];   // W | U | (V) | S as k_sqp_b / k_hom_b
  const int team = threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
  if (team >= kTeamsPerWave) return;   // the idle lanes of the wave (4 for teams of 5, 1 for teams of 9)
  const int i = blockIdx.x * kTeamsPerWave + team;
  if (i >= count) return;
  double* W = lds[team]; double* U = W + 81; double* V = WITH_V ? U + 81 : nullptr; double* S = U + (WITH_V ? 162 : 81);
  rsc::svd9_team<TEAM>(A + (size_t)i * 81, W, U, S, tl, V);
  double* o = out + (size_t)i * kSvdRecord;
  for (int e = tl; e < 9; e += TEAM) {
    for (int r = 0; r < 9; ++r) o[r * 9 + e] = U[r * 9 + e];
    o[81 + e] = S[e];
    if (WITH_V) for (int r = 0; r < 9; ++r) o[90 + r * 9 + e] = V[r * 9 + e];
  }
}
__global__ __launch_bounds__(64) void k_selftest_svd9_single(int count, const double* __restrict__ A, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  double* o = out + (size_t)i * kSvdRecord;
  rsc::svd_sq<9>(A + (size_t)i * 81, o, o + 81, o + 90);
}

// ---- five-point stage A.  Record per problem: ok | N [36] | M [100] (N and M untouched when ok = 0).
constexpr int kFpRecord = 137, kFpTeam = 16, kFpTeamsPerWave = 64 / kFpTeam;
__global__ __launch_bounds__(64, 4) void k_selftest_fp_pre_team(int count, const double* __restrict__ corr,
                                                                 const int* __restrict__ samples, double* __restrict__ out) {
  __shared__ double lds[kFpTeamsPerWave][rsc::kFit5TeamLds];
  const int team = threadIdx.x / kFpTeam, tl = threadIdx.x % kFpTeam;
  const int i = blockIdx.x * kFpTeamsPerWave + team;
  if (i >= count) return;
  double* o = out + (size_t)i * kFpRecord;
  const bool good = rsc::five_point_pre_team<kFpTeam>(corr, samples + (size_t)i * 5, lds[team], o + 1, o + 37, tl);
  if (tl == 0) o[0] = good ? 1.0 : 0.0;
}
__global__ __launch_bounds__(64) void k_selftest_fp_pre_single(int count, const double* __restrict__ corr, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  double* o = out + (size_t)i * kFpRecord;
  o[0] = rsc::five_point_pre(corr + (size_t)i * 20, o + 1, o + 37) ? 1.0 : 0.0;
}

constexpr int kMaxCount = 1 << 20;

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_selftest_eig_team(int32_t variant, int32_t n, int32_t count, const double* A, const int32_t* active,
                                           double* team_out, double* single_out) {
  const int lo = variant == 2 ? 10 : 1, hi = variant == 0 ? 10 : (variant == 1 ? 13 : 27);
  if (variant < 0 || variant > 2 || n < lo || n > hi)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "variant %d with n = %d (0: 1 .. 10, 1: 1 .. 13, 2: 10 .. 27)", variant, n);
  if (count < 1 || count > kMaxCount) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "count = %d", count);
  if (!A || !active || !team_out || !single_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  const size_t mats = (size_t)count * n * n, rec = eig_record(n) * count;
  DevBuf<double> d_A, d_work, d_work1, d_team, d_single; DevBuf<int> d_act;
  if ((rc = d_A.up(A, mats)) || (rc = d_work.up(A, mats)) || (rc = d_work1.alloc(mats)) || (rc = d_act.up(active, count)) ||
      (rc = d_team.up(team_out, rec)) || (rc = d_single.up(single_out, rec)))
    return rc;
  if (variant == 0) {
    k_selftest_eig_team<8, false, 0, 10, 1><<<(count + 7) / 8, 64, 0, nullptr>>>(n, count, d_act.p, d_work.p, d_team.p);
    HIP_TRY(hipGetLastError());
    k_selftest_eig_single<10, false><<<(count + 63) / 64, 64, 0, nullptr>>>(n, count, d_act.p, d_A.p, d_work1.p, d_single.p);
  } else if (variant == 1) {
    k_selftest_eig_team<8, true, 0, 13, 0><<<(count + 7) / 8, 64, 0, nullptr>>>(n, count, d_act.p, d_work.p, d_team.p);
    HIP_TRY(hipGetLastError());
    k_selftest_eig_single<13, true><<<(count + 63) / 64, 64, 0, nullptr>>>(n, count, d_act.p, d_A.p, d_work1.p, d_single.p);
  } else {
    k_selftest_eig_team<32, true, dlsdev::kKeptRows, 27, 2><<<(count + 1) / 2, 64, 0, nullptr>>>(n, count, d_act.p, d_work.p, d_team.p);
    HIP_TRY(hipGetLastError());
    k_selftest_eig_single<27, true><<<(count + 63) / 64, 64, 0, nullptr>>>(n, count, d_act.p, d_A.p, d_work1.p, d_single.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(team_out, d_team.p, sizeof(double) * rec, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(single_out, d_single.p, sizeof(double) * rec, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int theia_hip_selftest_svd9_team(int32_t team, int32_t with_v, int32_t count, const double* A, double* team_out,
                                            double* single_out) {
  if ((team != 5 && team != 9) || (with_v != 0 && with_v != 1))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "team = %d (5 or 9), with_v = %d (0 or 1)", team, with_v);
  if (count < 1 || count > kMaxCount) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "count = %d", count);
  if (!A || !team_out || !single_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  const size_t rec = (size_t)kSvdRecord * count;
  DevBuf<double> d_A, d_team, d_single;
  if ((rc = d_A.up(A, (size_t)81 * count)) || (rc = d_team.up(team_out, rec)) || (rc = d_single.up(single_out, rec))) return rc;
  const int tpw = 64 / team, blocks = (count + tpw - 1) / tpw;
  if (team == 5 && with_v) k_selftest_svd9_team<5, true><<<blocks, 64, 0, nullptr>>>(count, d_A.p, d_team.p);
  else if (team == 5) k_selftest_svd9_team<5, false><<<blocks, 64, 0, nullptr>>>(count, d_A.p, d_team.p);
  else if (with_v) k_selftest_svd9_team<9, true><<<blocks, 64, 0, nullptr>>>(count, d_A.p, d_team.p);
  else k_selftest_svd9_team<9, false><<<blocks, 64, 0, nullptr>>>(count, d_A.p, d_team.p);
  HIP_TRY(hipGetLastError());
  k_selftest_svd9_single<<<(count + 63) / 64, 64, 0, nullptr>>>(count, d_A.p, d_single.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(team_out, d_team.p, sizeof(double) * rec, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(single_out, d_single.p, sizeof(double) * rec, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int theia_hip_selftest_five_point_pre_team(int32_t count, const double* corr, double* team_out, double* single_out) {
  if (count < 1 || count > kMaxCount) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "count = %d", count);
  if (!corr || !team_out || !single_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  // the team reads its five correspondences through a sample list into one data array, as k_fit5_a_team does
  std::vector<int> samples((size_t)count * 5);
  for (size_t k = 0; k < samples.size(); ++k) samples[k] = (int)k;
  const size_t rec = (size_t)kFpRecord * count;
  DevBuf<double> d_corr, d_team, d_single; DevBuf<int> d_samples;
  if ((rc = d_corr.up(corr, (size_t)20 * count)) || (rc = d_samples.up(samples.data(), samples.size())) ||
      (rc = d_team.up(team_out, rec)) || (rc = d_single.up(single_out, rec)))
    return rc;
  k_selftest_fp_pre_team<<<(count + kFpTeamsPerWave - 1) / kFpTeamsPerWave, 64, 0, nullptr>>>(count, d_corr.p, d_samples.p, d_team.p);
  HIP_TRY(hipGetLastError());
  k_selftest_fp_pre_single<<<(count + 63) / 64, 64, 0, nullptr>>>(count, d_corr.p, d_single.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(team_out, d_team.p, sizeof(double) * rec, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(single_out, d_single.p, sizeof(double) * rec, hipMemcpyDeviceToHost));
  return 0;
}
