// pose_graph_sim3_check.cpp -- stand-alone host build of pytheiasfm_amd/csrc/pose_graph_sim3_device.h (the text the device
// compiles).  No HIP.  Reads records "op v0 v1 ..." from standard input and prints one line of %.17g values per record:
//   term   x_i[7] x_j[7] z[7] W[49]   -> ok residual[7] J_i[49]      (the weighted term)
//   term1  x_i[7] x_j[7] z[7]         -> ok residual[7] J_i[49]      (sqrt_information = identity, the NULL path)
//   plus   x[7] d[7]                  -> ok Plus(x, d)[7]
// Built and run by tests/test_pose_graph_sim3.py (-ffp-contract=off, as build.sh compiles the device side).
#include "pose_graph_sim3_device.h"

#include <cstdio>
#include <cstring>

namespace {
bool read(double* v, int n) {
  for (int k = 0; k < n; ++k)
    if (std::scanf("%lf", v + k) != 1) return false;
  return true;
}
void print(const double* v, int n) {
  for (int k = 0; k < n; ++k) std::printf(k + 1 < n ? "%.17g " : "%.17g\n", v[k]);
}
}  // namespace

int main() {
  using namespace thip::sim3;
  char op[16];
  while (std::scanf("%15s", op) == 1) {
    double in[70], out[57];
    for (double& v : out) v = 0.0;
    if (!std::strcmp(op, "term") || !std::strcmp(op, "term1")) {
      const bool weighted = !std::strcmp(op, "term");
      if (!read(in, weighted ? 70 : 21)) return 2;
      out[0] = pose_graph_term(in, in + 7, in + 14, weighted ? in + 21 : nullptr, out + 1, out + 8) ? 1.0 : 0.0;
      print(out, 57);
    } else if (!std::strcmp(op, "plus")) {
      if (!read(in, 14)) return 2;
      out[0] = pose_graph_plus(in, in + 7, out + 1) ? 1.0 : 0.0;
      print(out, 8);
    } else {
      return 3;
    }
  }
  return 0;
}
