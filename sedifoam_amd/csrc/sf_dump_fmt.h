// sf_dump_fmt.h -- exact "%g" (precision 6) and "%d" formatting of one value, for the dump kernels (sf_dump.hip).
//
// The bytes are those of glibc printf for every double: ±0, subnormals, inf / -inf / nan / -nan (the sign of a NaN is
// printed), the switch to exponent form at a decimal exponent < -4 or >= 6, trailing-zero removal, rounding that carries
// into the next exponent (9.999995 -> "10", 999999.5 -> "1e+06") and round-half-to-even on exact binary ties
// (1234565.0 -> "1.23456e+06").
//
// Method: a = |v| = m 2^e.  For a guess E of the decimal exponent, D = the integer nearest to a 10^(5-E) (ties to even) is
// found from a floating-point guess and exact comparisons sign(a 10^(5-E) - H/2) for integers H:
//   * |5-E| <= 22 (1e-17 <= a < 1e28: every physical value): 10^|5-E| is an exact double and fma(a, 10^k, -H/2) or
//     fma(-H/2, 10^k, a) is the correctly rounded difference, whose sign is the sign of the exact one;
//   * otherwise: the same comparison on integers, m 2^(e+1-j) 5^(-j) against H 5^j 2^(j-e-1) (j = E-5, every power on the
//     side where it is positive), at most ~820 bits.
// E is then moved by one while D is outside [1e5, 1e6).  No value is formatted by an inexact step.
//
// Compiles as HIP (host and device) or as plain C++ (SF_FMT_HD empty).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SF_FMT_HD __host__ __device__ inline
#else
#define SF_FMT_HD inline
#endif

namespace sf {
namespace fmt {

constexpr int kMaxG = 13;   // widest "%g" field: "-1.23457e-308"
constexpr int kMaxD = 11;   // widest "%d" field: "-2147483648"

// 10^k, k in [0, 22]: every product on the way is an exact double
SF_FMT_HD double pow10_exact(int k)
{
  double p = 1.0;
  for (int i = 0; i < k; i++) p *= 10.0;
  return p;
}

// unsigned integer of up to kBigWords 32-bit words, least significant first
constexpr int kBigWords = 28;   // 896 bits > the ~820 the widest comparison needs
struct Big {
  uint32_t w[kBigWords];
  int n;
};

SF_FMT_HD void big_set(Big& b, uint64_t v)
{
  b.w[0] = (uint32_t)v;
  b.w[1] = (uint32_t)(v >> 32);
  b.n = b.w[1] ? 2 : (b.w[0] ? 1 : 0);
}

SF_FMT_HD void big_mul32(Big& b, uint32_t f)
{
  uint64_t carry = 0;
  for (int i = 0; i < b.n; i++) {
    const uint64_t t = (uint64_t)b.w[i] * f + carry;
    b.w[i] = (uint32_t)t;
    carry = t >> 32;
  }
  if (carry && b.n < kBigWords) b.w[b.n++] = (uint32_t)carry;
}

SF_FMT_HD void big_mul_pow5(Big& b, int k)
{
  while (k >= 13) {
    big_mul32(b, 1220703125u);   // 5^13
    k -= 13;
  }
  uint32_t f = 1;
  for (int i = 0; i < k; i++) f *= 5u;
  if (f != 1) big_mul32(b, f);
}

SF_FMT_HD void big_shl(Big& b, int s)
{
  if (!b.n || s <= 0) return;
  const int ws = s >> 5, bs = s & 31;
  int n = b.n + ws + 1;
  if (n > kBigWords) n = kBigWords;   // (never reached: the operands stay below ~820 bits)
  for (int i = n - 1; i >= 0; i--) {
    const int src = i - ws;
    uint32_t hi = (src >= 0 && src < b.n) ? b.w[src] : 0u;
    uint32_t lo = (src - 1 >= 0 && src - 1 < b.n) ? b.w[src - 1] : 0u;
    b.w[i] = bs ? (hi << bs) | (lo >> (32 - bs)) : hi;
  }
  b.n = n;
  while (b.n && !b.w[b.n - 1]) b.n--;
}

SF_FMT_HD int big_cmp(const Big& a, const Big& b)
{
  if (a.n != b.n) return a.n < b.n ? -1 : 1;
  for (int i = a.n - 1; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}

// sign of a 10^(5-E) - H/2, exactly (a = m 2^e > 0, H >= 0)
SF_FMT_HD int cmp_scaled(double a, uint64_t m, int e, int E, int64_t H)
{
  const int k = 5 - E;
  const double h = 0.5 * (double)H;   // (H < 2^26: exact)
  if (k >= 0 && k <= 22) {
    const double r = fma(a, pow10_exact(k), -h);
    return (r > 0.0) - (r < 0.0);
  }
  if (k < 0 && k >= -22) {
    const double r = fma(-h, pow10_exact(-k), a);
    return (r > 0.0) - (r < 0.0);
  }
  // 2 a 10^k  vs  H, with j = -k:  m 2^(e+1) 5^(-j) 2^(-j)  vs  H
  const int j = -k, s = e + 1 - j;
  Big L, R;
  big_set(L, m);
  big_set(R, (uint64_t)H);
  if (j < 0) big_mul_pow5(L, -j);
  else big_mul_pow5(R, j);
  if (s > 0) big_shl(L, s);
  else big_shl(R, -s);
  return big_cmp(L, R);
}

// the integer nearest to a 10^(5-E), ties to even
SF_FMT_HD int64_t round_scaled(double a, uint64_t m, int e, int E)
{
  const int k = 5 - E;
  double y;
  if (k >= 0 && k <= 22) y = a * pow10_exact(k);
  else if (k < 0 && k >= -22) y = a / pow10_exact(-k);
  else {
    const int k1 = k / 2;   // (two factors: 10^k alone over- or underflows at the ends of the range)
    y = a * pow(10.0, (double)k1) * pow(10.0, (double)(k - k1));
  }
  if (!(y < 1e8)) y = 1e8;   // (E is a guess off by at most one: y stays far below this)
  int64_t D = (int64_t)floor(y);
  while (D > 0 && cmp_scaled(a, m, e, E, 2 * D) < 0) D--;   // now D <= a 10^k
  while (cmp_scaled(a, m, e, E, 2 * D + 2) >= 0) D++;       // now a 10^k < D + 1
  const int c = cmp_scaled(a, m, e, E, 2 * D + 1);
  if (c > 0 || (c == 0 && (D & 1))) D++;
  return D;
}

// "%g" of v into out (at most kMaxG bytes, no terminator); returns the length
SF_FMT_HD int format_g(double v, char* out)
{
  uint64_t bits;
  memcpy(&bits, &v, sizeof bits);
  const bool neg = bits >> 63;
  const int ef = (int)((bits >> 52) & 0x7ff);
  const uint64_t frac = bits & ((1ull << 52) - 1);
  char* p = out;
  if (neg) *p++ = '-';
  if (ef == 0x7ff) {
    const char* s = frac ? "nan" : "inf";
    for (int i = 0; i < 3; i++) *p++ = s[i];
    return (int)(p - out);
  }
  if (ef == 0 && frac == 0) {
    *p++ = '0';
    return (int)(p - out);
  }
  const uint64_t m = ef ? (frac | (1ull << 52)) : frac;
  const int e = ef ? ef - 1075 : -1074;
  const double a = fabs(v);
  // decimal exponent guess from the binary one, b = floor(log2 a): E or E - 1
  const int b = e + 63 - __builtin_clzll(m);
  int E = (int)floor((double)b * 0.30102999566398120);
  int64_t D = 0;
  for (int it = 0; it < 4; it++) {
    D = round_scaled(a, m, e, E);
    if (D >= 1000000) E++;        // a carry into the next decade, or the guess was one too low
    else if (D < 100000) E--;     // the guess was one too high
    else break;
  }
  char d[6];
  for (int i = 5; i >= 0; i--) {
    d[i] = (char)('0' + (int)(D % 10));
    D /= 10;
  }
  int last = 5;   // the last significant digit that is not a trailing zero
  while (last > 0 && d[last] == '0') last--;
  if (E < -4 || E >= 6) {
    *p++ = d[0];
    if (last > 0) {
      *p++ = '.';
      for (int i = 1; i <= last; i++) *p++ = d[i];
    }
    *p++ = 'e';
    *p++ = E < 0 ? '-' : '+';
    const int x = E < 0 ? -E : E;
    if (x >= 100) *p++ = (char)('0' + x / 100);
    *p++ = (char)('0' + (x / 10) % 10);
    *p++ = (char)('0' + x % 10);
  } else if (E >= 0) {
    for (int i = 0; i <= E; i++) *p++ = d[i];
    if (last > E) {
      *p++ = '.';
      for (int i = E + 1; i <= last; i++) *p++ = d[i];
    }
  } else {
    *p++ = '0';
    *p++ = '.';
    for (int i = 0; i < -E - 1; i++) *p++ = '0';
    for (int i = 0; i <= last; i++) *p++ = d[i];
  }
  return (int)(p - out);
}

// "%d" of v into out (at most kMaxD bytes); returns the length
SF_FMT_HD int format_d(int v, char* out)
{
  char* p = out;
  int64_t x = v;
  if (x < 0) {
    *p++ = '-';
    x = -x;
  }
  char t[10];
  int n = 0;
  do {
    t[n++] = (char)('0' + (int)(x % 10));
    x /= 10;
  } while (x);
  while (n) *p++ = t[--n];
  return (int)(p - out);
}

}  // namespace fmt
}  // namespace sf
