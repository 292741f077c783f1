// Generates golden RandGaussian streams with the REAL libstdc++ (std::mt19937 + std::normal_distribution<double>), i.e. what
// theia::RandomNumberGenerator::RandGaussian (src/theia/util/random.cc:87-91) executes: a fresh distribution object per call, so the
// second value of every polar pair is dropped.  The 1DSfM translation filter draws its projection axes this way
// (sfm/filter_view_pairs_from_relative_translation.cc:212-217).  Every row carries the generator's position after the draw: the
// number of 32-bit words taken since seeding (624 * regenerations + _M_p, read off operator<<), which pins the rejection loop.
// Build + run:  g++ -O2 -o /tmp/mk tests/golden/make_randgaussian_golden.cpp && /tmp/mk > tests/golden/mt19937_randgaussian.json
#include <cstdio>
#include <random>
#include <sstream>
#include <string>

static std::mt19937 gen;
static double RandGaussian(double mean, double std_dev) { std::normal_distribution<double> d(mean, std_dev); return d(gen); }
// _M_p: the last of the 625 numbers operator<< prints
static int Pos() {
  std::ostringstream os;
  os << gen;
  const std::string s = os.str();
  return std::stoi(s.substr(s.find_last_of(' ') + 1));
}

int main() {
  std::printf("{\n\"randgaussian\": [");
  const unsigned seeds[4] = {42u, 169u, 199u, 7u};
  const double params[5][2] = {{0.0, 1.0}, {-3.25, 0.5}, {0.125, 0.0}, {10.0, 0.03}, {-0.6, 2.0}};
  bool first = true;
  for (unsigned s : seeds) {
    gen.seed(s);
    long words = 0;
    int last = 624;   // _M_p right after seeding and after the last word of a block: the next draw regenerates
    for (int k = 0; k < 250; ++k) {
      const double* p = params[k % 5];
      const double v = RandGaussian(p[0], p[1]);
      const int pos = Pos();
      words += last == 624 ? pos : (pos > last ? pos - last : (624 - last) + pos);   // a draw takes far fewer than 624 words
      last = pos;
      std::printf("%s[%u,%.17g,%.17g,%.17g,%d,%ld]", first ? "" : ",", s, p[0], p[1], v, pos, words);
      first = false;
    }
  }
  std::printf("]\n}\n");
  return 0;
}
