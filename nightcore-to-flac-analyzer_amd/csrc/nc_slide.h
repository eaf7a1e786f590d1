// nc_slide.h — the tempogram autocorrelation as five sliding f64 sums.
//
// librosa.feature.tempogram (via beat_track's tempo estimate, tempo.py:45/63)
// autocorrelates every Hann-windowed frame of the ramp-padded onset envelope x:
//   ac_t[k] = sum_{j < N-k} w[j] w[j+k] x[t+j] x[t+j+k],   w = periodic Hann(N),
// normalises each frame by max_k |ac_t[k]| (= ac_t[0]) and averages over t
// (oracle/ncref.py tempogram_mean).  With theta = 2 pi / N the product of two
// shifted Hann windows is a trigonometric polynomial of degree 2 in j:
//   w[j] w[j+k] = A + B cos(theta j) + C sin(theta j) + D cos(2 theta j) + E sin(2 theta j)
//   A = 1/4 + c/8,  B = -1/4 - c/4,  C = s/4,  D = c/8,  E = -s/8,   (c, s) = (cos, sin)(theta k).
// With p_k[u] = x[u] x[u+k] and L = N - k this gives
//   ac_t[k] = A S0(t) + B Re Z1(t) + C Im Z1(t) + D Re Z2(t) + E Im Z2(t),
//   S0(t) = sum_{j<L} p_k[t+j],   Zm(t) = sum_{j<L} e^{i m theta j} p_k[t+j],
// and every sum slides one frame in O(1):
//   Zm(t+1) = e^{-i m theta} (Zm(t) - p_k[t] + e^{i m theta L} p_k[t+L]),  e^{i m theta L} = e^{-i m theta k}.
// All arithmetic is f64: about 28 flops per (lag, frame), against two 2N-point
// FFTs per frame.  Agreement with librosa's f64 FFT autocorrelation is at the 1e-15
// level while the envelope keeps a bounded dynamic range between two seeds
// (tests/test_oracle_known_answers.py checks the identity) -- and only then.  The sums
// are slid by subtraction, so their rounding residue is proportional to the loudest
// passage they have held, while the normaliser 1 / ac_t[0] follows the current frame:
// once the envelope falls to exact zero (every mel band under the top_db clamp: a gap, a
// fade to digital silence), the frames that still see the last samples under the far tail
// of the Hann window (weight ~ (pi j / N)^4) divide that residue by an ac_t[0] twelve or
// more decades smaller, and the mean is off by 1e-3 and more.  Remedy (slide_lag_sum[2]): the
// five sums are recomputed directly (slide_seed) at every frame whose ac_t[0] has fallen
// below SLIDE_RESEED = 2^-20 of the largest one since the last seed -- two or three extra
// seeds per fall, an error near 1e-7 at the worst instead (tests/tempo_feature_cases.py
// restates the rule, tests/test_gpu_tempo_features.py holds the kernels to it).  ac_t[0] is
// the same for every lag, so all threads of a block re-seed at the same frames, and the
// decision uses frames of the current [t0, t1) only: a tile's row does not depend on which
// launch computes it.
#pragma once
#include <hip/hip_runtime.h>

namespace nc {

// Per-lag state of the sliding sums (see the header comment).
struct SlideLag {
  double A, B, C, D, E;      // w[j] w[j+k] expansion coefficients
  double ck, sk, ck2, sk2;   // e^{-i theta k}, e^{-2 i theta k} (= e^{i m theta L})
  double S0, z1r, z1i, z2r, z2i;
  int k, L;
};

// the five sums of frame t, directly
template <class XF>
__device__ __forceinline__ void slide_seed(SlideLag& s, const XF& x, int N, int t, double c1, double s1) {
  const double inv_half = 2.0 / (double)N;
  const int k = s.k;
  double S0 = 0.0, z1r = 0.0, z1i = 0.0, z2r = 0.0, z2i = 0.0;
  for (int j0 = 0; j0 < s.L; j0 += 64) {
    double es, ec;  // e^{i theta j}, re-seeded every 64 terms
    sincospi((double)j0 * inv_half, &es, &ec);
    const int je = min(s.L, j0 + 64);
    for (int j = j0; j < je; ++j) {
      const double p = (double)x(t + j) * (double)x(t + j + k);
      const double e2c = fma(ec, ec, -es * es), e2s = 2.0 * ec * es;
      S0 += p;
      z1r = fma(ec, p, z1r);
      z1i = fma(es, p, z1i);
      z2r = fma(e2c, p, z2r);
      z2i = fma(e2s, p, z2i);
      const double nc = fma(ec, c1, -es * s1), ns = fma(es, c1, ec * s1);
      ec = nc;
      es = ns;
    }
  }
  s.S0 = S0;
  s.z1r = z1r;
  s.z1i = z1i;
  s.z2r = z2r;
  s.z2i = z2i;
}

__device__ __forceinline__ void slide_coeffs(SlideLag& s, int N, int k) {
  const double inv_half = 2.0 / (double)N;
  double sk, ck;
  sincospi((double)k * inv_half, &sk, &ck);
  s.k = k;
  s.L = N - k;
  s.ck = ck;
  s.sk = sk;
  s.ck2 = fma(ck, ck, -sk * sk);
  s.sk2 = 2.0 * ck * sk;
  s.A = 0.25 + 0.125 * ck;
  s.B = -0.25 - 0.25 * ck;
  s.C = 0.25 * sk;
  s.D = 0.125 * ck;
  s.E = -0.125 * sk;
}

__device__ __forceinline__ double slide_ac(const SlideLag& s) {
  return fma(s.E, s.z2i, fma(s.D, s.z2r, fma(s.C, s.z1i, fma(s.B, s.z1r, s.A * s.S0))));
}

// advance one frame given p[t] and p[t + L]
__device__ __forceinline__ void slide_step(SlideLag& s, double pt, double pl, double c1, double s1, double c2,
                                           double s2) {
  s.S0 = (s.S0 - pt) + pl;
  const double u1r = fma(s.ck, pl, s.z1r - pt), u1i = fma(-s.sk, pl, s.z1i);
  s.z1r = fma(u1r, c1, u1i * s1);
  s.z1i = fma(u1i, c1, -u1r * s1);
  const double u2r = fma(s.ck2, pl, s.z2r - pt), u2i = fma(-s.sk2, pl, s.z2i);
  s.z2r = fma(u2r, c2, u2i * s2);
  s.z2i = fma(u2i, c2, -u2r * s2);
}

// ac_t[0] below this fraction of the largest one since the last seed: seed again
constexpr double SLIDE_RESEED = 1.0 / 1048576.0;  // 2^-20

// sum_{t0 <= t < t1} ac_t[k] * rinv(t); x(i) returns the padded envelope (float), valid for
// t0 <= i <= t1 - 1 + N.  The frames are walked in runs: each run starts from directly
// computed sums (slide_seed) and slides until the re-seeding rule of the header comment ends
// it.  rmin is the smallest rinv (largest ac_t[0]) of the run; frames whose ac_t[0] is below
// tiny (rinv = 1, tg_rinv) neither end a run nor count.
template <class XF, class RF>
__device__ __forceinline__ double slide_lag_sum(const XF& x, const RF& rinv, int N, int k, int t0, int t1) {
  double s1, c1;
  sincospi(2.0 / (double)N, &s1, &c1);
  const double c2 = fma(c1, c1, -s1 * s1), s2 = 2.0 * c1 * s1;
  SlideLag a;
  slide_coeffs(a, N, k);
  double acc = 0.0;
  int t = t0;
  while (t < t1) {
    slide_seed(a, x, N, t, c1, s1);
    // operands of frame t are loaded one frame ahead (software pipelining: the LDS latency
    // overlaps the previous frame's arithmetic); x must be readable up to t1 - 1 + N
    double xt = (double)x(t), xk = (double)x(t + k), xl = (double)x(t + a.L), xn = (double)x(t + N);
    double r = rinv(t), rmin = r != 1.0 ? r : INFINITY;
    for (;;) {
      const int tn = t + 1 < t1 ? t + 1 : t;
      const double xt1 = (double)x(tn), xk1 = (double)x(tn + k), xl1 = (double)x(tn + a.L), xn1 = (double)x(tn + N);
      const double r1 = rinv(tn);
      acc = fma(slide_ac(a), r, acc);
      slide_step(a, xt * xk, xl * xn, c1, s1, c2, s2);
      xt = xt1;
      xk = xk1;
      xl = xl1;
      xn = xn1;
      r = r1;
      if (++t >= t1) break;
      if (r != 1.0) {
        if (r * SLIDE_RESEED > rmin) break;
        rmin = fmin(rmin, r);
      }
    }
  }
  return acc;
}

// Two lags at once (independent dependency chains interleaved; the x(t) and rinv(t)
// reads are shared).  Same arithmetic per lag, same runs as slide_lag_sum.
template <class XF, class RF>
__device__ __forceinline__ void slide_lag_sum2(const XF& x, const RF& rinv, int N, int ka, int kb, int t0, int t1,
                                               double& acc_a, double& acc_b) {
  double s1, c1;
  sincospi(2.0 / (double)N, &s1, &c1);
  const double c2 = fma(c1, c1, -s1 * s1), s2 = 2.0 * c1 * s1;
  SlideLag a, b;
  slide_coeffs(a, N, ka);
  slide_coeffs(b, N, kb);
  double ra = 0.0, rb = 0.0;
  int t = t0;
  while (t < t1) {
    slide_seed(a, x, N, t, c1, s1);
    slide_seed(b, x, N, t, c1, s1);
    // operands loaded one frame ahead (see slide_lag_sum)
    double xt = (double)x(t), xn = (double)x(t + N), xka = (double)x(t + ka), xkb = (double)x(t + kb);
    double xla = (double)x(t + a.L), xlb = (double)x(t + b.L), r = rinv(t), rmin = r != 1.0 ? r : INFINITY;
    for (;;) {
      const int tn = t + 1 < t1 ? t + 1 : t;
      const double xt1 = (double)x(tn), xn1 = (double)x(tn + N), xka1 = (double)x(tn + ka), xkb1 = (double)x(tn + kb);
      const double xla1 = (double)x(tn + a.L), xlb1 = (double)x(tn + b.L), r1 = rinv(tn);
      ra = fma(slide_ac(a), r, ra);
      rb = fma(slide_ac(b), r, rb);
      slide_step(a, xt * xka, xla * xn, c1, s1, c2, s2);
      slide_step(b, xt * xkb, xlb * xn, c1, s1, c2, s2);
      xt = xt1;
      xn = xn1;
      xka = xka1;
      xkb = xkb1;
      xla = xla1;
      xlb = xlb1;
      r = r1;
      if (++t >= t1) break;
      if (r != 1.0) {
        if (r * SLIDE_RESEED > rmin) break;
        rmin = fmin(rmin, r);
      }
    }
  }
  acc_a = ra;
  acc_b = rb;
}

// Normaliser of one frame: 1 / ac_t[0] (librosa util.normalize(norm=inf) with
// threshold tiny(f64): a frame whose max is below tiny is left as is).
__device__ __forceinline__ double tg_rinv(double ac0) { return ac0 < 2.2250738585072014e-308 ? 1.0 : 1.0 / ac0; }

}  // namespace nc
