// The shim's RandomNumberGenerator and RansacParameters::rng (bundle_adjuster_hip.h): the state against a real std::mt19937
// (draws, Import / Export), then -- unless --host-only -- estimates that share one generator, as a reference pipeline does.
// Prints "ok ..." per check; exit status 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "bundle_adjuster_hip.h"

using namespace theia_hip_shim;

static void rotate(const double w[3], const double v[3], double out[3]) {   // angle-axis rotation (Rodrigues)
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (th < 1e-15) { std::memcpy(out, v, 3 * sizeof(double)); return; }
  const double k[3] = {w[0] / th, w[1] / th, w[2] / th}, c = std::cos(th), s = std::sin(th);
  const double kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
  const double kx[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
  for (int i = 0; i < 3; ++i) out[i] = v[i] * c + kx[i] * s + k[i] * kv * (1 - c);
}

static bool same(const RandomNumberGenerator& a, const RandomNumberGenerator& b) {
  return std::memcmp(a.state()->mt, b.state()->mt, sizeof(a.state()->mt)) == 0 && a.state()->pos == b.state()->pos;
}

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && std::string(argv[1]) == "--host-only";
  // ---- the generator against libstdc++
  RandomNumberGenerator rng(65);
  std::mt19937 ref(65);
  for (int i = 0; i < 2000; ++i) {
    std::uniform_int_distribution<int> di(i % 7, 1999 + i);
    std::uniform_real_distribution<double> dd(-0.5, 0.5);
    if (rng.RandInt(i % 7, 1999 + i) != di(ref) || rng.RandDouble(-0.5, 0.5) != dd(ref)) { std::printf("FAIL: draws differ at %d\n", i); return 1; }
  }
  std::mt19937 out;
  rng.Export(&out);
  if (!(out == ref)) { std::printf("FAIL: Export\n"); return 1; }
  for (int i = 0; i < 700; ++i) (void)ref();
  RandomNumberGenerator imp(1);
  imp.Import(ref);
  std::uniform_int_distribution<int> d(0, 99);
  for (int i = 0; i < 50; ++i) if (imp.RandInt(0, 99) != d(ref)) { std::printf("FAIL: Import\n"); return 1; }
  std::printf("ok generator state against std::mt19937\n");
  if (host_only) return 0;

  // ---- relative pose: four pairs in one batch on one generator = four calls in turn on another
  std::mt19937 gen(11);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  std::vector<std::vector<double>> corr(4);
  for (int p = 0; p < 4; ++p) {
    const double w[3] = {0.1 * U(gen), 0.2 * U(gen), 0.1 * U(gen)};
    double t[3] = {U(gen), 0.3 * U(gen), 0.2 * U(gen)};
    const double tn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (double& x : t) x /= tn;
    for (int i = 0; i < 300; ++i) {
      const double X[3] = {2 * U(gen), 2 * U(gen), 6 + 2 * U(gen)};
      const double dv[3] = {X[0] - t[0], X[1] - t[1], X[2] - t[2]};
      double q[3];
      rotate(w, dv, q);
      double x1 = X[0] / X[2], y1 = X[1] / X[2], x2 = q[0] / q[2], y2 = q[1] / q[2];
      if (i % (3 + p) == 0) { x2 = U(gen); y2 = U(gen); }
      else { x1 += 5e-4 * N(gen); y1 += 5e-4 * N(gen); x2 += 5e-4 * N(gen); y2 += 5e-4 * N(gen); }
      corr[p].insert(corr[p].end(), {x1, y1, x2, y2});
    }
  }
  RansacParameters rp;
  rp.error_thresh = 2.5e-3 * 2.5e-3; rp.min_iterations = 20; rp.max_iterations = 2000;
  rp.rng = std::make_shared<RandomNumberGenerator>(7);
  std::vector<bool> ok; std::vector<RelativePose> poses; std::vector<RansacSummary> sums; std::string err;
  if (!EstimateRelativePoseBatch(rp, corr, &ok, &poses, &sums, &err)) { std::printf("FAIL: %s\n", err.c_str()); return 1; }
  RansacParameters one = rp;
  one.rng = std::make_shared<RandomNumberGenerator>(7);
  for (int p = 0; p < 4; ++p) {
    std::vector<bool> ok1; std::vector<RelativePose> pose1; std::vector<RansacSummary> sum1;
    if (!EstimateRelativePoseBatch(one, {corr[p]}, &ok1, &pose1, &sum1, &err)) { std::printf("FAIL: %s\n", err.c_str()); return 1; }
    if (ok1[0] != ok[p] || sum1[0].inliers != sums[p].inliers || sum1[0].num_iterations != sums[p].num_iterations ||
        std::memcmp(pose1[0].rotation, poses[p].rotation, sizeof(poses[p].rotation)) != 0) {
      std::printf("FAIL: pair %d differs between the chained batch and the call on its own\n", p);
      return 1;
    }
  }
  if (!same(*rp.rng, *one.rng)) { std::printf("FAIL: the generators end in different states\n"); return 1; }
  // the generator moved by exactly the reference's draws: RandomSampler, five RandInt per iteration on a fresh permutation
  std::mt19937 chk(7);
  for (int p = 0; p < 4; ++p) {
    std::vector<int> idx(300);
    for (int i = 0; i < 300; ++i) idx[i] = i;
    for (int it = 0; it < sums[p].num_iterations; ++it)
      for (int i = 0; i < 5; ++i) { std::uniform_int_distribution<int> di(i, 299); std::swap(idx[i], idx[di(chk)]); }
  }
  std::mt19937 end;
  rp.rng->Export(&end);
  if (!(end == chk)) { std::printf("FAIL: the generator is not where the reference's would stand\n"); return 1; }
  std::printf("ok relative pose on a shared generator (iterations %d %d %d %d)\n", sums[0].num_iterations, sums[1].num_iterations,
              sums[2].num_iterations, sums[3].num_iterations);
  return 0;
}
