// ba_query.hip -- the entry points that read a BA handle without running a solve: evaluation of residuals and Jacobians,
// the covariance blocks, the reduced system of one linearisation, and the dense SPD solve the tests call directly.
#include <cmath>
#include <cstdio>
#include <string>

#include "ba_handle.h"

extern "C" {

// One line per kernel family a run() of the handle launches, from the helpers the launch sites branch on (ba_kernels.h).
int theia_hip_ba_kernel_instances(theia_ba_handle h, char* buf, int32_t cap) {
  if (!h || !buf || cap <= 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  std::string out;
  auto line = [&out](const char* fmt, auto... a) { char t[160]; snprintf(t, sizeof(t), fmt, a...); out += t; out += '\n'; };
  auto models = [](bool trig) { return trig ? "all" : "notrig"; };
  if (h->idh) {
    line("inverse_depth");
  } else {
    const DevProblem& P = h->P;
    const LinRoute route = linearize_route(P);
    if (route == LIN_FUSED) {
      const FusedInstance f = lin_schur_instance(P);
      line("k_lin_schur pd=%d models=%s lossk=%d first=0", f.pd, models(f.trig), f.lossk);
      if (scale_fold_applies(h)) line("k_lin_schur pd=%d models=%s lossk=%d first=1", f.pd, models(f.trig), f.lossk);
      if (backsub_runs_applies(P)) {
        const FusedInstance b = backsub_runs_instance(P);
        line("k_backsub_runs pd=%d models=%s lossk=%d waves=%d intr=0 kmask=0", b.pd, models(b.trig), b.lossk, b.waves);
      } else line("k_backsub pd=%d intr=0 rot=1", P.pd);
    } else if (route == LIN_FUSED_INTR) {
      const FusedInstance f = lin_schur_intr_instance(P);
      line("k_lin_schur_i pd=%d models=%s lossk=%d bw=%d kmask=%d", f.pd, models(f.trig), f.lossk, f.bw, (int)f.kmask);
      if (backsub_runs_intr_applies(P)) {
        const FusedInstance b = backsub_runs_intr_instance(P);
        line("k_backsub_runs pd=%d models=%s lossk=%d waves=%d intr=1 kmask=%d", b.pd, models(b.trig), b.lossk, b.waves, (int)b.kmask);
      } else line("k_backsub pd=%d intr=1 rot=1", P.pd);
    } else if (route == LIN_GATHER_INTR) {
      line("k_lin_obs_intr pd=%d ki=%d", P.pd, P.intr_rows == 4 ? 4 : 10);
      line("k_backsub pd=%d intr=1 rot=0", P.pd);
    } else if (route == LIN_GATHER) {
      line("k_lin_obs pd=%d", P.pd);
      line("k_backsub pd=%d intr=0 rot=0", P.pd);
    }
    if (P.long_nobs > 0) line("k_long pd=%d intr=%d", P.pd, P.ni ? 1 : 0);
    if (h->inner && h->opt.use_inner_iterations != 0) {
      const InnerInstance i = inner_instance(P);
      if (P.nc > 0) line("k_inner_views models=%s lossk=%d priors=%d", models(!i.lean), i.lean ? i.lossk1 : 2, (int)i.priors);
      if (P.ni > 0 && P.ng_total > 0) line("k_inner_groups models=%s lossk=%d kc=%d", models(!i.lean), i.lean ? i.lossk1 : 2, i.kc);
      if (P.ntiles > 0) line("k_inner_tracks pd=%d models=%s lossk=%d", i.pd, models(i.trig), i.lossk);
    }
  }
  if ((size_t)cap <= out.size()) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "kernel_instances: buffer too small");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return 0;
}

int theia_hip_ba_lm_chain(theia_ba_handle h, int32_t* folded) {
  if (!h || !folded) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *folded = (!h->idh && lm_glue_run(h)) ? 1 : 0;
  return 0;
}

int theia_hip_ba_evaluate(theia_ba_handle h, double* cost, double* residuals, double* jac_cam, double* jac_pt, uint8_t* valid) {
  return theia_hip_ba_evaluate_ex(h, cost, residuals, jac_cam, jac_pt, nullptr, valid);
}

int theia_hip_ba_evaluate_ex(theia_ba_handle h, double* cost, double* residuals, double* jac_cam, double* jac_pt,
                             double* jac_intr, uint8_t* valid) {
  if (h && h->idh) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "inverse-depth handle: evaluate is not built in this mode");
  if (!h) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle");
  release_stage_if_idle(h);
  const int pd = h->pd;
  PoolBuf<double> dr, djc, djp, dji; PoolBuf<uint8_t> dv;
  int rc;
  const size_t nm = (size_t)h->nobs_main;
  if ((rc = dr.alloc(2 * nm)) || (rc = djc.alloc(12 * nm)) || (rc = djp.alloc(2 * pd * nm)) || (rc = dv.alloc(nm))) return rc;
  const bool want_ji = jac_intr && h->ni;
  if (want_ji && (rc = dji.alloc(20 * nm))) return rc;
  DevProblem Q = h->P;
  Q.scale_c = h->ones_c.p; Q.scale_p = h->ones_p.p;
  Q.ntiles = h->ntiles_eval;
  Q.scale_i = h->ones_i.p; Q.intr = h->intr[h->cur].p;
  HIP_TRYR(hipMemsetAsync(h->scalB.p, 0, sizeof(double) * 16, h->stream));
  launch_evaluate(Q, h->cam[h->cur].p, h->pts[h->cur].p, dr.p, djc.p, djp.p, dv.p, h->tile_part.p, h->stream, want_ji ? dji.p : nullptr);
  if (h->ntiles_eval) launch_reduce_tiles(h->ntiles_eval, h->tile_part.p, 2, h->f2s.p + 16, h->fmaxflag.p + 16, h->scalB.p, h->stream);
  launch_cam_priors(Q, PRIOR_COST, h->cam[h->cur].p, nullptr, nullptr, nullptr, nullptr, h->scalB.p + SB_COST, nullptr, h->stream);
  std::vector<double> hr(2 * nm), hjc(12 * nm), hjp(2 * pd * nm); std::vector<uint8_t> hv(nm);
  if (nm) {
    HIP_TRYR(hipMemcpyAsync(hr.data(), dr.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRYR(hipMemcpyAsync(hjc.data(), djc.p, sizeof(double) * hjc.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRYR(hipMemcpyAsync(hjp.data(), djp.p, sizeof(double) * hjp.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRYR(hipMemcpyAsync(hv.data(), dv.p, hv.size(), hipMemcpyDeviceToHost, h->stream));
  }
  std::vector<double> hji;
  if (want_ji && nm) { hji.resize(20 * nm); HIP_TRYR(hipMemcpyAsync(hji.data(), dji.p, sizeof(double) * hji.size(), hipMemcpyDeviceToHost, h->stream)); }
  HIP_TRYR(hipMemcpyAsync(h->h_scal + 16, h->scalB.p, sizeof(double) * 16, hipMemcpyDeviceToHost, h->stream));
  HIP_TRYR(hipStreamSynchronize(h->stream));
  if (cost) *cost = h->h_scal[16 + SB_COST] + h->fixed_cost;
  if (jac_intr) std::fill(jac_intr, jac_intr + 20 * h->nobs, 0.0);
  if (want_ji) for (size_t s2 = 0; s2 < nm; ++s2) std::copy(&hji[20 * s2], &hji[20 * s2] + 20, jac_intr + 20 * h->perm[s2]);
  if (residuals) std::fill(residuals, residuals + 2 * h->nobs, 0.0);
  if (jac_cam) std::fill(jac_cam, jac_cam + 12 * h->nobs, 0.0);
  if (jac_pt) std::fill(jac_pt, jac_pt + 2 * pd * h->nobs, 0.0);
  if (valid) std::fill(valid, valid + h->nobs, (uint8_t)1);
  for (size_t s = 0; s < nm; ++s) {
    const int64_t i = h->perm[s];
    if (residuals) { residuals[2 * i] = hr[2 * s]; residuals[2 * i + 1] = hr[2 * s + 1]; }
    if (jac_cam) std::copy(&hjc[12 * s], &hjc[12 * s] + 12, jac_cam + 12 * i);
    if (jac_pt) std::copy(&hjp[2 * pd * s], &hjp[2 * pd * s] + 2 * pd, jac_pt + 2 * pd * i);
    if (valid) valid[i] = hv[s];
  }
  release_stage_if_idle(h);
  return 0;
}

// Covariance blocks of the two block-diagonal cases the reference exposes (GetCovarianceFor{Track,Tracks,View,Views},
// bundle_adjuster.cc:660-773, behind the *WithCov entry points bundle_adjustment.cc:288-386,420-499): tracks against
// constant cameras (3x3 / 4x4 in the point's tangent space) and views against constant tracks (6x6).  In both the
// normal matrix J'J is block diagonal, so ceres::Covariance's (J'J)^-1 is the inverse of each block.  J is the
// loss-corrected, unscaled Jacobian at the current state (Covariance::Options::apply_loss_function = true).
int theia_hip_ba_covariance(theia_ba_handle h, double* point_cov, double* cam_cov) {
  if (h && h->idh) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "inverse-depth handle: covariance is not built in this mode");
  if (!h) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle");
  release_stage_if_idle(h);
  if (!point_cov && !cam_cov) return 0;
  // Optimised intrinsics couple the cameras of a group: J'J of the views problem is an arrow per group, not block diagonal
  // (handled below by the arrow's Schur complement, linear in the number of cameras).
  // (point covariances on a handle with optimised intrinsics: not a case the reference can produce -- BundleAdjustTrack(s)
  // holds every camera constant and with them the intrinsics groups, bundle_adjuster.cc:204-212 -- refused)
  if (h->ni && point_cov) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "point covariances with optimised intrinsics: BundleAdjustTrack(s) keeps all intrinsics constant (bundle_adjuster.cc:204-212)");
  bool any_var_point = false;
  for (int q = 0; q < h->np; ++q) any_var_point |= !h->pt_const[q];
  if (point_cov && h->ncv > 0)
    return set_error(THEIA_HIP_ERR_UNSUPPORTED, "point covariances need all cameras constant (the BundleAdjustTrack(s) problem)");
  if (cam_cov && any_var_point)
    return set_error(THEIA_HIP_ERR_UNSUPPORTED, "camera covariances need all points constant (the BundleAdjustView(s) problem)");
  if (cam_cov)
    for (int c = 0; c < h->nc; ++c)
      if (h->cam_red[c] >= 0 && h->cam_mask[c]) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "covariance of a partially constant camera");
  const int pd = h->pd, NT = pd * (pd + 1) / 2;
  DevProblem Q = h->P;
  Q.scale_c = h->ones_c.p; Q.scale_p = h->ones_p.p; Q.scale_i = h->ones_i.p; Q.intr = h->intr[h->cur].p;
  Q.camrot_current = 0; h->camrot_valid = false;   // (the per-camera blocks are rebuilt with the unit scales, and are the solve's no longer)
  LmState st;
  std::memset(&st, 0, sizeof(st));
  st.radius = 1e300;   // no LM damping: D = clamp(diag) / radius vanishes against the diagonal
  HIP_TRYR(hipMemcpyAsync(h->lm_state.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
  HIP_TRYR(hipStreamSynchronize(h->stream));
  const double* radius = &reinterpret_cast<const LmState*>(h->lm_state.p)->radius;
  HIP_TRYR(hipMemsetAsync(h->reduce.p, 0, sizeof(double) * h->reduce.n, h->stream));
  if (h->Vinv.n) HIP_TRYR(hipMemsetAsync(h->Vinv.p, 0, sizeof(double) * h->Vinv.n, h->stream));
  launch_linearize(Q, h->cam[h->cur].p, h->pts[h->cur].p, radius, h->rb, h->Vinv.p, h->gp.p, h->tile_part.p, h->stream);
  launch_long_linearize(Q, h->cam[h->cur].p, h->pts[h->cur].p, radius, h->rb, h->Vinv.p, h->gp.p, h->long_scratch.p, h->stream);
  if (point_cov) {
    std::vector<double> vi((size_t)NT * h->np);
    if (h->np) HIP_TRYR(hipMemcpyAsync(vi.data(), h->Vinv.p, sizeof(double) * vi.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRYR(hipStreamSynchronize(h->stream));
    for (int q = 0; q < h->np; ++q)
      for (int a = 0; a < pd; ++a)
        for (int b = 0; b < pd; ++b)
          point_cov[(size_t)q * pd * pd + a * pd + b] = vi[(size_t)NT * q + (a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a)];
  }
  if (cam_cov) {
    const int n = h->n;
    std::vector<double> S((size_t)n * n);
    if (n) HIP_TRYR(hipMemcpyAsync(S.data(), h->rb.S, sizeof(double) * S.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRYR(hipStreamSynchronize(h->stream));
    std::fill(cam_cov, cam_cov + 36 * (size_t)h->nc, 0.0);
    if (h->ni) {
      // Optimised intrinsics: with every point constant J'J is an ARROW per intrinsics group -- [G_g  B^T; B  D], D block diagonal
      // over the group's cameras (6 x 6 each), G_g the group's 10 x 10 block -- and groups do not couple.  The extrinsics block
      // of camera c of (J'J)^-1 is   D_c^-1 + Y_c (G_g - sum_c' B_c'^T D_c'^-1 B_c')^-1 Y_c^T,   Y_c = D_c^-1 B_c :
      // work linear in the number of cameras, no limit on the size of the reduced system (the dense host factorisation of the
      // earlier rounds stopped at 2048 columns).  Slots of parameters outside the optimised subset are empty rows: left out.
      const int ni = h->ni;
      std::vector<double> G((size_t)ni * 10);   // [group][10][10] lower triangle mirrored
      for (int i = 0; i < ni; ++i)
        for (int j = 0; j < 10; ++j) { const int gs = 10 * (i / 10), r = std::max(i, gs + j), q = std::min(i, gs + j); G[(size_t)i * 10 + j] = S[(size_t)r * n + q]; }
      std::vector<int> cg((size_t)std::max(1, h->nc));
      if (h->nc) HIP_TRYR(hipMemcpy(cg.data(), h->cam_group.p, sizeof(int) * h->nc, hipMemcpyDeviceToHost));
      auto chol_inv = [](const double* A, int m, double* Ainv) -> bool {   // inverse of an SPD m x m matrix (m <= 10), row-major
        double L[100], Li[100];
        for (int i = 0; i < m; ++i)
          for (int j = 0; j <= i; ++j) {
            double v = A[i * m + j];
            for (int k = 0; k < j; ++k) v -= L[i * m + k] * L[j * m + k];
            if (i == j) { if (!(v > 0.0)) return false; L[i * m + i] = std::sqrt(v); }
            else L[i * m + j] = v / L[j * m + j];
          }
        for (int i = 0; i < m; ++i) {
          for (int j = 0; j < m; ++j) Li[i * m + j] = 0.0;
          Li[i * m + i] = 1.0 / L[i * m + i];
          for (int j = 0; j < i; ++j) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v -= L[i * m + k] * Li[k * m + j];
            Li[i * m + j] = v / L[i * m + i];
          }
        }
        for (int a = 0; a < m; ++a)
          for (int b = 0; b < m; ++b) {
            double v = 0.0;
            for (int k = std::max(a, b); k < m; ++k) v += Li[k * m + a] * Li[k * m + b];
            Ainv[a * m + b] = v;
          }
        return true;
      };
      const int ngv = ni / 10;
      // per camera: D_c^-1 and Y_c = D_c^-1 B_c (6 x 10); per group: the Schur complement onto its intrinsics
      std::vector<double> Dinv((size_t)36 * h->nc, 0.0), Y((size_t)60 * h->nc, 0.0), SG(G);
      for (int c = 0; c < h->nc; ++c) {
        const int rc = h->cam_red[c];
        if (rc < 0) continue;
        const int o = ni + 6 * rc, gr = h->grp_red[cg[c]];
        double D[36];
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) D[a * 6 + b] = S[(size_t)(o + std::max(a, b)) * n + o + std::min(a, b)];
        if (!chol_inv(D, 6, &Dinv[(size_t)36 * c])) return set_error(THEIA_HIP_ERR_INTERNAL, "camera %d: J'J is rank deficient (ceres::Covariance::Compute fails)", c);
        if (gr < 0) continue;
        double* Yc = &Y[(size_t)60 * c];
        for (int a = 0; a < 6; ++a)
          for (int k = 0; k < 10; ++k) {
            double v = 0.0;
            for (int b = 0; b < 6; ++b) v += Dinv[(size_t)36 * c + a * 6 + b] * S[(size_t)(o + b) * n + 10 * gr + k];
            Yc[a * 10 + k] = v;
          }
        for (int k = 0; k < 10; ++k)
          for (int l = 0; l < 10; ++l) {
            double v = 0.0;
            for (int a = 0; a < 6; ++a) v += S[(size_t)(o + a) * n + 10 * gr + k] * Yc[a * 10 + l];
            SG[(size_t)(10 * gr + k) * 10 + l] -= v;
          }
      }
      std::vector<double> SGinv((size_t)ni * 10, 0.0);   // [group][10][10], zero rows / columns at the empty slots
      for (int gr = 0; gr < ngv; ++gr) {
        int act[10], na = 0;
        for (int k = 0; k < 10; ++k) if (G[(size_t)(10 * gr + k) * 10 + k] != 0.0) act[na++] = k;
        if (!na) continue;
        double A[100], Ai[100];
        for (int a = 0; a < na; ++a)
          for (int b = 0; b < na; ++b) A[a * na + b] = SG[(size_t)(10 * gr + act[a]) * 10 + act[b]];
        if (!chol_inv(A, na, Ai)) return set_error(THEIA_HIP_ERR_INTERNAL, "J'J is rank deficient in intrinsics group slot %d (ceres::Covariance::Compute fails)", gr);
        for (int a = 0; a < na; ++a)
          for (int b = 0; b < na; ++b) SGinv[(size_t)(10 * gr + act[a]) * 10 + act[b]] = Ai[a * na + b];
      }
      for (int c = 0; c < h->nc; ++c) {
        const int rc = h->cam_red[c];
        if (rc < 0) continue;
        const int gr = h->grp_red[cg[c]];
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) {
            double v = Dinv[(size_t)36 * c + a * 6 + b];
            if (gr >= 0) {
              const double* Yc = &Y[(size_t)60 * c];
              for (int k = 0; k < 10; ++k) {
                double t = 0.0;
                for (int l = 0; l < 10; ++l) t += SGinv[(size_t)(10 * gr + k) * 10 + l] * Yc[b * 10 + l];
                v += Yc[a * 10 + k] * t;
              }
            }
            cam_cov[(size_t)c * 36 + a * 6 + b] = v;
          }
      }
      release_stage_if_idle(h);
      return 0;
    }
    for (int c = 0; c < h->nc; ++c) {
      const int rc = h->cam_red[c];
      if (rc < 0) continue;
      double L[36], Li[36];
      bool ok = true;
      for (int i = 0; i < 6 && ok; ++i)
        for (int j = 0; j <= i; ++j) {
          double s = S[(size_t)(6 * rc + i) * n + 6 * rc + j];
          for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k];
          if (i == j) { if (!(s > 0.0)) { ok = false; break; } L[i * 6 + i] = std::sqrt(s); }
          else L[i * 6 + j] = s / L[j * 6 + j];
        }
      if (!ok) return set_error(THEIA_HIP_ERR_INTERNAL, "camera %d: J'J is rank deficient (ceres::Covariance::Compute fails)", c);
      for (int i = 0; i < 6; ++i) {   // Li = L^-1
        for (int j = 0; j < 6; ++j) Li[i * 6 + j] = 0.0;
        Li[i * 6 + i] = 1.0 / L[i * 6 + i];
        for (int j = 0; j < i; ++j) {
          double s = 0.0;
          for (int k = j; k < i; ++k) s -= L[i * 6 + k] * Li[k * 6 + j];
          Li[i * 6 + j] = s / L[i * 6 + i];
        }
      }
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
          double s = 0.0;
          for (int k = std::max(a, b); k < 6; ++k) s += Li[k * 6 + a] * Li[k * 6 + b];
          cam_cov[(size_t)c * 36 + a * 6 + b] = s;
        }
    }
  }
  release_stage_if_idle(h);
  return 0;
}

int theia_hip_dense_spd_solve(int32_t n, const double* A, const double* b, double* x) {
  if (n < 0 || (n > 0 && (!A || !b || !x))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (n == 0) return 0;
  int rc = thip::ensure_device();
  if (rc) return rc;
  PoolBuf<double> dA, dw, dflag;
  if ((rc = dA.alloc((size_t)n * n + n)) || (rc = dw.alloc(dense_cholesky_workspace(n))) || (rc = dflag.alloc(1))) return rc;
  HIP_TRYR(hipMemcpy(dA.p, A, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice));
  HIP_TRYR(hipMemcpy(dA.p + (size_t)n * n, b, sizeof(double) * n, hipMemcpyHostToDevice));
  HIP_TRYR(hipMemset(dflag.p, 0, sizeof(double)));
  dense_cholesky_solve(n, dA.p, n, dA.p + (size_t)n * n, dw.p, dflag.p, nullptr);
  double flag = 0.0;
  if (getenv("THEIA_HIP_DEBUG_FACTOR")) {  // development aid: hand back the factor in place of A
    HIP_TRYR(hipMemcpy(const_cast<double*>(A), dA.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
  }
  HIP_TRYR(hipMemcpy(x, dA.p + (size_t)n * n, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIP_TRYR(hipMemcpy(&flag, dflag.p, sizeof(double), hipMemcpyDeviceToHost));
  if (flag != 0.0) return set_error(THEIA_HIP_ERR_INTERNAL, "matrix is not positive definite");
  return 0;
}

int theia_hip_ba_reduced_system(theia_ba_handle h, double radius, int32_t* n_out, double* S, double* rhs, int64_t capacity) {
  if (h && h->idh) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "inverse-depth handle: the reduced-system dump is not built in this mode");
  if (!h || !n_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const bool fold = scale_fold_applies(h);   // the route run() takes for its first linearisation
  int rc = fold ? 0 : compute_scale(h);
  if (rc) return rc;
  {
    LmState st;
    std::memset(&st, 0, sizeof(st));
    st.radius = radius;
    HIP_TRYR(hipMemcpyAsync(h->lm_state.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
    HIP_TRYR(hipStreamSynchronize(h->stream));   // `st` is a stack object
  }
  rc = enqueue_linearize(h, 0, fold);
  if (rc) return rc;
  const int n = h->n;
  *n_out = n;
  if ((int64_t)n * n > capacity) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "capacity too small for %d x %d", n, n);
  HIP_TRYR(hipStreamSynchronize(h->stream));
  if (n) {
    HIP_TRYR(hipMemcpy(S, h->rb.S, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
    HIP_TRYR(hipMemcpy(rhs, h->rb.rhs, sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) S[(size_t)i * n + j] = S[(size_t)j * n + i];
  return 0;
}

}  // extern "C"
