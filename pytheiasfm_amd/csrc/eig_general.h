// eig_general.h -- real general eigen-decomposition and companion-matrix polynomial roots on the device (gfx950, FP64),
// one thread per matrix.  Restates the published algorithm behind the Eigen call of the reference:
//   Eigen::EigenSolver (five_point_relative_pose.cc:275; companion-matrix
//                       roots, math/find_polynomial_roots_companion_matrix.cc)
//                      = EISPACK orthes + hqr2
// Built with -ffp-contract=off: the operation order below is kept identical to
// the CPU oracle's transcription of the same algorithms, which is what makes
// RANSAC inlier sets bit-identical between the two (DESIGN.md "RANSAC parity").
#pragma once
#include <hip/hip_runtime.h>

#include "small_linalg.h"   // RDEV

namespace thip {
namespace rsc {

// Real general eigen-decomposition (EISPACK orthes + hqr2, as in JAMA) of an
// n x n row-major matrix, n <= 10.  H is destroyed.  wr/wi: eigenvalues; if V
// is non-null it receives the (un-normalised) eigenvectors of the REAL
// eigenvalues in the corresponding columns (row-major n x n).
// complex division (xr + i xi) / (yr + i yi), Smith's scaling (EISPACK cdiv)
RDEV void eig_cdiv(double xr, double xi, double yr, double yi, double* cr, double* ci) {
  if (fabs(yr) > fabs(yi)) {
    const double r = yi / yr, d = yr + r * yi;
    *cr = (xr + r * xi) / d; *ci = (xi - r * xr) / d;
  } else {
    const double r = yr / yi, d = yi + r * yr;
    *cr = (r * xr + xi) / d; *ci = (r * xi - xr) / d;
  }
}
const int EIG_MAXN = 10;
// MAXN: largest n of the instantiation (sizes the one local array).  CPLX: also back-substitute the complex
// conjugate pairs (EISPACK hqr2 convention: for wi[j] > 0 the columns j, j + 1 of V hold the real and the
// imaginary part of the eigenvector of wr[j] + i wi[j]; the DLS solver reads them, dls_pnp.cc:147-161).
template <int MAXN, bool CPLX>
RDEV bool eig_general_t(int nn, double* H, double* wr, double* wi, double* V) {
#define HH(i, j) H[(i) * nn + (j)]
#define VV(i, j) V[(i) * nn + (j)]
  const int low = 0, high = nn - 1;
  double ort[MAXN];
  // ---- orthes: reduce to Hessenberg form
  for (int m = low + 1; m <= high - 1; ++m) {
    double scale = 0.0;
    for (int i = m; i <= high; ++i) scale += fabs(HH(i, m - 1));
    if (scale != 0.0) {
      double h = 0.0;
      for (int i = high; i >= m; --i) { ort[i] = HH(i, m - 1) / scale; h += ort[i] * ort[i]; }
      double g = sqrt(h);
      if (ort[m] > 0) g = -g;
      h = h - ort[m] * g;
      ort[m] = ort[m] - g;
      for (int j = m; j < nn; ++j) {
        double f = 0.0;
        for (int i = high; i >= m; --i) f += ort[i] * HH(i, j);
        f = f / h;
        for (int i = m; i <= high; ++i) HH(i, j) -= f * ort[i];
      }
      for (int i = 0; i <= high; ++i) {
        double f = 0.0;
        for (int j = high; j >= m; --j) f += ort[j] * HH(i, j);
        f = f / h;
        for (int j = m; j <= high; ++j) HH(i, j) -= f * ort[j];
      }
      ort[m] = scale * ort[m];
      HH(m, m - 1) = scale * g;
    } else {
      ort[m] = 0.0;
    }
  }
  if (V) {
    for (int i = 0; i < nn; ++i) for (int j = 0; j < nn; ++j) VV(i, j) = (i == j) ? 1.0 : 0.0;
    for (int m = high - 1; m >= low + 1; --m) {
      if (HH(m, m - 1) != 0.0) {
        for (int i = m + 1; i <= high; ++i) ort[i] = HH(i, m - 1);
        for (int j = m; j <= high; ++j) {
          double g = 0.0;
          for (int i = m; i <= high; ++i) g += ort[i] * VV(i, j);
          g = (g / ort[m]) / HH(m, m - 1);
          for (int i = m; i <= high; ++i) VV(i, j) += g * ort[i];
        }
      }
    }
  }
  // ---- hqr2
  int n = nn - 1;
  const double eps = 2.220446049250313e-16;
  double exshift = 0.0;
  double p = 0, q = 0, r = 0, s = 0, z = 0, t, w, x, y;
  double norm = 0.0;
  for (int i = 0; i < nn; ++i)
    for (int j = (i - 1 > 0 ? i - 1 : 0); j < nn; ++j) norm += fabs(HH(i, j));
  if (norm == 0.0) {   // the zero matrix: every deflation test would read 0 < eps * 0 and the sweeps run on 0 / 0
    for (int i = 0; i < nn; ++i) { wr[i] = 0.0; wi[i] = 0.0; }
    return true;        // V: the accumulation's identity
  }
  int iter = 0, total_iter = 0;
  while (n >= low) {
    int l = n;
    while (l > low) {
      s = fabs(HH(l - 1, l - 1)) + fabs(HH(l, l));
      if (s == 0.0) s = norm;
      if (fabs(HH(l, l - 1)) < eps * s) break;
      l--;
    }
    if (l == n) {  // one root
      HH(n, n) = HH(n, n) + exshift;
      wr[n] = HH(n, n); wi[n] = 0.0;
      n--; iter = 0;
    } else if (l == n - 1) {  // two roots
      w = HH(n, n - 1) * HH(n - 1, n);
      p = (HH(n - 1, n - 1) - HH(n, n)) / 2.0;
      q = p * p + w;
      z = sqrt(fabs(q));
      HH(n, n) = HH(n, n) + exshift;
      HH(n - 1, n - 1) = HH(n - 1, n - 1) + exshift;
      x = HH(n, n);
      if (q >= 0) {  // real pair
        z = (p >= 0) ? p + z : p - z;
        wr[n - 1] = x + z;
        wr[n] = wr[n - 1];
        if (z != 0.0) wr[n] = x - w / z;
        wi[n - 1] = 0.0; wi[n] = 0.0;
        x = HH(n, n - 1);
        s = fabs(x) + fabs(z);
        p = x / s; q = z / s;
        r = sqrt(p * p + q * q);
        p = p / r; q = q / r;
        for (int j = n - 1; j < nn; ++j) { z = HH(n - 1, j); HH(n - 1, j) = q * z + p * HH(n, j); HH(n, j) = q * HH(n, j) - p * z; }
        for (int i = 0; i <= n; ++i) { z = HH(i, n - 1); HH(i, n - 1) = q * z + p * HH(i, n); HH(i, n) = q * HH(i, n) - p * z; }
        if (V) for (int i = low; i <= high; ++i) { z = VV(i, n - 1); VV(i, n - 1) = q * z + p * VV(i, n); VV(i, n) = q * VV(i, n) - p * z; }
      } else {  // complex pair
        wr[n - 1] = x + p; wr[n] = x + p; wi[n - 1] = z; wi[n] = -z;
      }
      n = n - 2; iter = 0;
    } else {
      x = HH(n, n); y = 0.0; w = 0.0;
      if (l < n) { y = HH(n - 1, n - 1); w = HH(n, n - 1) * HH(n - 1, n); }
      if (iter == 10) {  // Wilkinson's original ad hoc shift
        exshift += x;
        for (int i = low; i <= n; ++i) HH(i, i) -= x;
        s = fabs(HH(n, n - 1)) + fabs(HH(n - 1, n - 2));
        x = y = 0.75 * s;
        w = -0.4375 * s * s;
      }
      if (iter == 30) {  // MATLAB's new ad hoc shift
        s = (y - x) / 2.0;
        s = s * s + w;
        if (s > 0) {
          s = sqrt(s);
          if (y < x) s = -s;
          s = x - w / ((y - x) / 2.0 + s);
          for (int i = low; i <= n; ++i) HH(i, i) -= s;
          exshift += s;
          x = y = w = 0.964;
        }
      }
      iter = iter + 1;
      if (++total_iter > 40 * nn) return false;  // Eigen: m_maxIterationsPerRow * size
      int m = n - 2;
      while (m >= l) {
        z = HH(m, m);
        r = x - z; s = y - z;
        p = (r * s - w) / HH(m + 1, m) + HH(m, m + 1);
        q = HH(m + 1, m + 1) - z - r - s;
        r = HH(m + 2, m + 1);
        s = fabs(p) + fabs(q) + fabs(r);
        p = p / s; q = q / s; r = r / s;
        if (m == l) break;
        if (fabs(HH(m, m - 1)) * (fabs(q) + fabs(r)) <
            eps * (fabs(p) * (fabs(HH(m - 1, m - 1)) + fabs(z) + fabs(HH(m + 1, m + 1))))) break;
        m--;
      }
      for (int i = m + 2; i <= n; ++i) { HH(i, i - 2) = 0.0; if (i > m + 2) HH(i, i - 3) = 0.0; }
      for (int k = m; k <= n - 1; ++k) {
        const bool notlast = (k != n - 1);
        if (k != m) {
          p = HH(k, k - 1); q = HH(k + 1, k - 1);
          r = notlast ? HH(k + 2, k - 1) : 0.0;
          x = fabs(p) + fabs(q) + fabs(r);
          if (x == 0.0) continue;
          p = p / x; q = q / x; r = r / x;
        }
        s = sqrt(p * p + q * q + r * r);
        if (p < 0) s = -s;
        if (s != 0) {
          if (k != m) HH(k, k - 1) = -s * x;
          else if (l != m) HH(k, k - 1) = -HH(k, k - 1);
          p = p + s; x = p / s; y = q / s; z = r / s; q = q / p; r = r / p;
          for (int j = k; j < nn; ++j) {
            p = HH(k, j) + q * HH(k + 1, j);
            if (notlast) { p = p + r * HH(k + 2, j); HH(k + 2, j) = HH(k + 2, j) - p * z; }
            HH(k, j) = HH(k, j) - p * x;
            HH(k + 1, j) = HH(k + 1, j) - p * y;
          }
          const int imax = (n < k + 3) ? n : k + 3;
          for (int i = 0; i <= imax; ++i) {
            p = x * HH(i, k) + y * HH(i, k + 1);
            if (notlast) { p = p + z * HH(i, k + 2); HH(i, k + 2) = HH(i, k + 2) - p * r; }
            HH(i, k) = HH(i, k) - p;
            HH(i, k + 1) = HH(i, k + 1) - p * q;
          }
          if (V) for (int i = low; i <= high; ++i) {
            p = x * VV(i, k) + y * VV(i, k + 1);
            if (notlast) { p = p + z * VV(i, k + 2); VV(i, k + 2) = VV(i, k + 2) - p * r; }
            VV(i, k) = VV(i, k) - p;
            VV(i, k + 1) = VV(i, k + 1) - p * q;
          }
        }
      }
    }
  }
  if (!V) return true;
  // back-substitution for the REAL eigenvectors of the quasi-triangular form
  for (n = nn - 1; n >= 0; --n) {
    p = wr[n]; q = wi[n];
    if (CPLX && q < 0 && n > 0) {   // second member of a conjugate pair: columns n - 1 (real part) and n (imaginary part)
      int l = n - 1;
      if (fabs(HH(n, n - 1)) > fabs(HH(n - 1, n))) {
        HH(n - 1, n - 1) = q / HH(n, n - 1);
        HH(n - 1, n) = -(HH(n, n) - p) / HH(n, n - 1);
      } else {
        double cr, ci;
        eig_cdiv(0.0, -HH(n - 1, n), HH(n - 1, n - 1) - p, q, &cr, &ci);
        HH(n - 1, n - 1) = cr; HH(n - 1, n) = ci;
      }
      HH(n, n - 1) = 0.0; HH(n, n) = 1.0;
      double lastra = 0.0, lastsa = 0.0, lastw = 0.0;
      for (int i = n - 2; i >= 0; --i) {
        double ra = 0.0, sa = 0.0;
        for (int j = l; j <= n; ++j) { ra = ra + HH(i, j) * HH(j, n - 1); sa = sa + HH(i, j) * HH(j, n); }
        w = HH(i, i) - p;
        if (wi[i] < 0.0) { lastw = w; lastra = ra; lastsa = sa; continue; }
        l = i;
        double cr, ci;
        if (wi[i] == 0.0) {
          eig_cdiv(-ra, -sa, w, q, &cr, &ci);
          HH(i, n - 1) = cr; HH(i, n) = ci;
        } else {
          x = HH(i, i + 1); y = HH(i + 1, i);
          double vr = (wr[i] - p) * (wr[i] - p) + wi[i] * wi[i] - q * q;
          const double vi = (wr[i] - p) * 2.0 * q;
          if (vr == 0.0 && vi == 0.0) vr = eps * norm * (fabs(w) + fabs(q) + fabs(x) + fabs(y) + fabs(lastw));
          eig_cdiv(x * lastra - lastw * ra + q * sa, x * lastsa - lastw * sa - q * ra, vr, vi, &cr, &ci);
          HH(i, n - 1) = cr; HH(i, n) = ci;
          if (fabs(x) > (fabs(lastw) + fabs(q))) {
            HH(i + 1, n - 1) = (-ra - w * HH(i, n - 1) + q * HH(i, n)) / x;
            HH(i + 1, n) = (-sa - w * HH(i, n) - q * HH(i, n - 1)) / x;
          } else {
            eig_cdiv(-lastra - y * HH(i, n - 1), -lastsa - y * HH(i, n), lastw, q, &cr, &ci);
            HH(i + 1, n - 1) = cr; HH(i + 1, n) = ci;
          }
        }
        t = fmax(fabs(HH(i, n - 1)), fabs(HH(i, n)));
        if ((eps * t) * t > 1) for (int j = i; j <= n; ++j) { HH(j, n - 1) = HH(j, n - 1) / t; HH(j, n) = HH(j, n) / t; }
      }
      continue;
    }
    if (q != 0) continue;
    int l = n;
    HH(n, n) = 1.0;
    for (int i = n - 1; i >= 0; --i) {
      w = HH(i, i) - p;
      r = 0.0;
      for (int j = l; j <= n; ++j) r = r + HH(i, j) * HH(j, n);
      if (wi[i] < 0.0) { z = w; s = r; }
      else {
        l = i;
        if (wi[i] == 0.0) {
          if (w != 0.0) HH(i, n) = -r / w;
          else HH(i, n) = -r / (eps * norm);
        } else {
          x = HH(i, i + 1); y = HH(i + 1, i);
          q = (wr[i] - p) * (wr[i] - p) + wi[i] * wi[i];
          t = (x * s - z * r) / q;
          HH(i, n) = t;
          if (fabs(x) > fabs(z)) HH(i + 1, n) = (-r - w * t) / x;
          else HH(i + 1, n) = (-s - y * t) / z;
        }
        t = fabs(HH(i, n));
        if ((eps * t) * t > 1) for (int j = i; j <= n; ++j) HH(j, n) = HH(j, n) / t;
      }
    }
  }
  // back transformation (only the real-eigenvalue columns are meaningful)
  for (int j = nn - 1; j >= low; --j) {
    if (!CPLX && wi[j] != 0) continue;
    for (int i = low; i <= high; ++i) {
      z = 0.0;
      for (int k = low; k <= j; ++k) z = z + VV(i, k) * HH(k, j);
      VV(i, j) = z;
    }
  }
  return true;
#undef HH
#undef VV
}
RDEV bool eig_real_general(int nn, double* H, double* wr, double* wi, double* V) {
  return eig_general_t<EIG_MAXN, false>(nn, H, wr, wi, V);
}

// math/find_polynomial_roots_companion_matrix.cc for degree >= 3 (the quartic
// of P3P): normalise, companion matrix, power-of-two balancing (gamma = 0.9),
// eigenvalues; REAL PARTS of all roots are returned (reference quirk).
RDEV int poly_roots_real_parts(const double* poly_in, int size, double* real_out) {
  int lead = 0;
  while (lead < size - 1 && poly_in[lead] == 0) ++lead;  // RemoveLeadingZeros
  const double* poly = poly_in + lead;
  const int degree = size - lead - 1;
  if (degree == 0) return 0;
  if (degree == 1) { real_out[0] = -poly[1] / poly[0]; return 1; }
  if (degree == 2) {  // FindQuadraticPolynomialRoots (math/polynomial.cc)
    const double a = poly[0], b = poly[1], c = poly[2];
    const double D = b * b - 4 * a * c;
    const double sqrt_D = sqrt(fabs(D));
    if (D >= 0) {
      if (b >= 0) { real_out[0] = (-b - sqrt_D) / (2.0 * a); real_out[1] = (2.0 * c) / (-b - sqrt_D); }
      else { real_out[0] = (2.0 * c) / (-b + sqrt_D); real_out[1] = (-b + sqrt_D) / (2.0 * a); }
    } else { real_out[0] = -b / (2.0 * a); real_out[1] = -b / (2.0 * a); }
    return 2;
  }
  double p[EIG_MAXN + 1];
  for (int i = 0; i <= degree; ++i) p[i] = poly[i] / poly[0];
  double Cm[EIG_MAXN * EIG_MAXN];
  for (int i = 0; i < degree * degree; ++i) Cm[i] = 0.0;
  for (int i = 1; i < degree; ++i) Cm[i * degree + i - 1] = 1.0;
  for (int i = 0; i < degree; ++i) Cm[i * degree + degree - 1] = -p[degree - i];
  // BalanceCompanionMatrix
  {
    double Off[EIG_MAXN * EIG_MAXN];
    for (int i = 0; i < degree * degree; ++i) Off[i] = Cm[i];
    for (int i = 0; i < degree; ++i) Off[i * degree + i] = 0.0;
    const double gamma = 0.9;
    bool changed;
    do {
      changed = false;
      for (int i = 0; i < degree; ++i) {
        double row_norm = 0.0, col_norm = 0.0;
        for (int j = 0; j < degree; ++j) { row_norm += fabs(Off[i * degree + j]); col_norm += fabs(Off[j * degree + i]); }
        int exponent = 0;
        frexp(row_norm / col_norm, &exponent);
        exponent /= 2;
        if (exponent != 0) {
          const double scaled_col = ldexp(col_norm, exponent);
          const double scaled_row = ldexp(row_norm, -exponent);
          if (scaled_col + scaled_row < gamma * (col_norm + row_norm)) {
            changed = true;
            const double rs = ldexp(1.0, -exponent), cs = ldexp(1.0, exponent);
            for (int j = 0; j < degree; ++j) Off[i * degree + j] *= rs;
            for (int j = 0; j < degree; ++j) Off[j * degree + i] *= cs;
          }
        }
      }
    } while (changed);
    for (int i = 0; i < degree; ++i) Off[i * degree + i] = Cm[i * degree + i];
    for (int i = 0; i < degree * degree; ++i) Cm[i] = Off[i];
  }
  double wr[EIG_MAXN], wi[EIG_MAXN];
  if (!eig_real_general(degree, Cm, wr, wi, nullptr)) return 0;
  for (int i = 0; i < degree; ++i) real_out[i] = wr[i];
  return degree;
}

}  // namespace rsc
}  // namespace thip
