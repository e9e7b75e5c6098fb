// The seven idf columns of one frequency family (include/mi355det.h, "Dataset statistics"), as plain double arithmetic that compiles for the
// device and, without hipcc, for the host (tests/test_idf_host.py runs it against scipy).  yolo/utilities/custom.py:221-242 of the reference.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define MI355_HD __host__ __device__ inline
#else
#define MI355_HD inline
#endif

namespace mi355 {

// Inverse of the normal distribution function: the rational approximations of Cephes' ndtri.c, which scipy.special.ndtri evaluates
// (S. L. Moshier, Cephes Math Library 2.1).  Coefficients highest power first; the Q polynomials are monic (Cephes' p1evl).
MI355_HD double ndtri_polevl(double x, const double* c, int n) {
  double r = c[0];
  for (int i = 1; i <= n; ++i) r = r * x + c[i];
  return r;
}
MI355_HD double ndtri_p1evl(double x, const double* c, int n) {
  double r = x + c[0];
  for (int i = 1; i < n; ++i) r = r * x + c[i];
  return r;
}

MI355_HD double ndtri(double y0) {
  // central region, |y - 0.5| <= 3/8 in Cephes' words: exp(-2) < y < 1 - exp(-2)
  const double P0[5] = {-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1, 1.39312609387279679503E1,
                        -1.23916583867381258016E0};
  const double Q0[8] = {1.95448858338141759834E0, 4.67627912898881538453E0,  8.63602421390890590575E1, -2.25462687854119370527E2,
                        2.00260212380060660359E2, -8.20372256168333339912E1, 1.59056225126211695515E1, -1.18331621121330003142E0};
  // tails: z = sqrt(-2 log y) between 2 and 8
  const double P1[9] = {4.05544892305962419923E0,   3.15251094599893866154E1,   5.71628192246421288162E1,
                        4.40805073893200834700E1,   1.46849561928858024014E1,   2.18663306850790267539E0,
                        -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4};
  const double Q1[8] = {1.57799883256466749731E1, 4.53907635128879210584E1,   4.13172038254672030440E1,   1.50425385692907503408E1,
                        2.50464946208309415979E0, -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4};
  // z between 8 and 64
  const double P2[9] = {3.23774891776946035970E0,  6.91522889068984211695E0,  3.93881025292474443415E0,
                        1.33303460815807542389E0,  2.01485389549179081538E-1, 1.23716634817820021358E-2,
                        3.01581553508235416007E-4, 2.65806974686737550832E-6, 6.23974539184983293730E-9};
  const double Q2[8] = {6.02427039364742014255E0,  3.67983563856160859403E0,  1.37702099489081330271E0,  2.16236993594496635890E-1,
                        1.34204006088543189037E-2, 3.28014464682127739104E-4, 2.89247864745380683936E-6, 6.79019408009981274425E-9};
  const double s2pi = 2.50662827463100050242E0;        // sqrt(2 pi)
  const double expm2 = 0.13533528323661269189;         // exp(-2)
  if (y0 == 0.0) return -INFINITY;
  if (y0 == 1.0) return INFINITY;
  if (!(y0 > 0.0 && y0 < 1.0)) return NAN;
  bool negate = true;
  double y = y0;
  if (y > 1.0 - expm2) {
    y = 1.0 - y;
    negate = false;
  }
  if (y > expm2) {
    y = y - 0.5;
    const double y2 = y * y;
    const double x = y + y * (y2 * ndtri_polevl(y2, P0, 4) / ndtri_p1evl(y2, Q0, 8));
    return x * s2pi;
  }
  double x = sqrt(-2.0 * log(y));
  const double x0 = x - log(x) / x;
  const double z = 1.0 / x;
  const double x1 = x < 8.0 ? z * ndtri_polevl(z, P1, 8) / ndtri_p1evl(z, Q1, 8) : z * ndtri_polevl(z, P2, 8) / ndtri_p1evl(z, Q2, 8);
  x = x0 - x1;
  return negate ? -x : x;
}

// One family: total = the number of documents (images, or all instances), freq = this category's count of them, both exact in double.
// out[0..6] = smooth, raw, prob, normit, gombit, base2, base10.  freq == total gives p = 1: prob, normit and gombit are -inf, as in numpy.
MI355_HD void idf_columns(double total, double freq, double* out) {
  const double p = freq / total;
  out[0] = log((total + 1.0) / (freq + 1.0)) + 1.0;
  out[1] = log(total / freq);
  out[2] = log((total - freq) / freq);
  out[3] = -ndtri(p);
  out[4] = -log(-log(1.0 - p));
  out[5] = -log2(p);
  out[6] = -log10(p);
}

}  // namespace mi355
