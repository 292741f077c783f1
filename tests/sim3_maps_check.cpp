// sim3_maps_check.cpp -- stand-alone host build of pytheiasfm_amd/csrc/sim3_device.h (the text the device compiles).  No HIP.
// Reads records "op v0 v1 ..." from standard input and prints the map's result, one line of %.17g values per record:
//   exp   a[7]               -> sR[9] t[3]
//   expd  a[7]               -> sR[9] t[3] dsR[9][7] dt[3][7]
//   log   scale R[9] t[3]    -> ok a[7]
//   from  R[9] t[3] scale    -> ok a[7]
//   to    a[7]               -> R[9] t[3] scale
//   mat   a[7]               -> M[16]
// Built and run by tests/test_sim3_alignment.py (-ffp-contract=off, as build.sh compiles the device side).
#include "sim3_device.h"

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
    double in[13], out[96];
    if (!std::strcmp(op, "exp")) {
      if (!read(in, 7)) return 2;
      sim3_exp(in, out, out + 9);
      print(out, 12);
    } else if (!std::strcmp(op, "expd")) {
      if (!read(in, 7)) return 2;
      sim3_exp_d(in, out, out + 9, out + 12, out + 75);
      print(out, 96);
    } else if (!std::strcmp(op, "log")) {
      if (!read(in, 13)) return 2;
      out[0] = sim3_log(in[0], in + 1, in + 10, out + 1) ? 1.0 : 0.0;
      print(out, 8);
    } else if (!std::strcmp(op, "from")) {
      if (!read(in, 13)) return 2;
      out[0] = sim3_from_rts(in, in + 9, in[12], out + 1) ? 1.0 : 0.0;
      print(out, 8);
    } else if (!std::strcmp(op, "to")) {
      if (!read(in, 7)) return 2;
      sim3_to_rts(in, out, out + 9, out + 12);
      print(out, 13);
    } else if (!std::strcmp(op, "mat")) {
      if (!read(in, 7)) return 2;
      sim3_to_matrix4(in, out);
      print(out, 16);
    } else {
      return 3;
    }
  }
  return 0;
}
