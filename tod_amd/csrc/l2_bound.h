// The float matcher's filter bound (l2.hip's head comment, include/todhip.h): THE statement of the bf16 rounding of a component and
// of eps(q), the distance between the bf16 GEMM's score and the defining f32 d2. l2_prepare_kernel evaluates these functions on the
// device and nothing else in the library restates the constants; tests/l2_bound_host_test.cpp includes this header into a host
// program and holds the inequality against binary64 on worst-case and random inputs. Plain C++.
//
//   score(q, r) = |r|^2 - 2 <q^, r^>                       q^, r^: every component rounded to bf16 (l2_bf16_rne)
//   |score(q, r) + |q|^2 - d2(q, r)| <= eps(q)             d2: the sequential f32 sum of include/todhip.h, |q|^2 the exact norm
//   eps(q) = kL2EpsLead |q| Rmax + kL2EpsSum (|q| + Rmax)^2        Rmax = max |r| over the DB
//
// Derivation. u = 2^-8: bf16 keeps 8 significant bits, so round-to-nearest-even moves a component x by at most u |x| (1 + 2^-8 - 2^-22
// rounds to 1). q^ = q + a and r^ = r + b with |a_i| <= u |q_i|, |b_i| <= u |r_i|, and in exact arithmetic
//   score + |q|^2 - (|q|^2 + |r|^2 - 2 <q, r>) = -2 (<a, r> + <q, b> + <a, b>),
//   |<a, r>| <= u sum |q_i| |r_i| <= u |q| |r|   (Cauchy-Schwarz), likewise <q, b>;   |<a, b>| <= u^2 |q| |r|:
//   the bf16 term is at most (4 u + 2 u^2) |q| |r| = 2^-6 (1 + 2^-9) |q| |r|, and inputs exist that come within 2^-8 of it (all a_i r_i
//   and q_i b_i of one sign, every component just beside a rounding boundary: the host test's worst-case families).
// kL2EpsLead = 2^-6 (1 + 2^-6). The 2^-6 relative on top of 4 u holds the cross term (2^-9), the f32 evaluation of eps itself from f32
// norms (a shuffle-tree sum and two sqrtf: below 2^-20) and bf16 subnormal components, whose error is absolute (2^-134 each, nothing
// beside a |q| of at least 2^-63); the rest, 2^-6 - 2^-9 - 2^-20, is margin that no known input uses.
// kL2EpsSum = 2^-14 holds every f32 rounding, each relative to a partial sum that (|q| + Rmax)^2 bounds:
//   the sequential f32 sum that DEFINES d2 (a rounded difference, a rounded square, 127 rounded additions: < 2^-17 d2, d2 <= (|q| + |r|)^2);
//   |r|^2 as the prepare kernel leaves it (one product, one addition, six shuffle steps: < 2^-21 |r|^2);
//   the matrix cores' f32 accumulation of the 128 exact bf16 x bf16 products onto |r|^2 (136 additions of at most one ulp each, 2^-23,
//   of a partial sum below |r|^2 + 2 |q^| |r^|: < 2^-15.9 (|q| + Rmax)^2);
//   together below 2^-15 (|q| + Rmax)^2 -- half of the term. The other half covers the f32 rounding of the threshold A_k + 2 eps.
// Rows of 64 floats (desc_bytes 256) use the same two constants. No term grows when the width shrinks: the bf16 term is
// Cauchy-Schwarz and does not know the dimension; the defining sum has 63 rounded additions instead of 127, the matrix cores accumulate
// 72 times instead of 136, and the narrow prepare kernel's norm is one product and the six shuffle steps without the addition in front.
// tests/l2_dim64_bound_host_test.cpp holds the inequality at 64 dimensions against binary64 (worst-case families: 0.97 of eps).
// Domain: finite components, |q|^2 and every |r|^2 normal f32 numbers (no overflow, no underflow). The bound is relative and says
// nothing once a norm has underflowed.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TOD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TOD_HD inline
#endif

namespace tod {

constexpr float kL2EpsLead = 0.015869140625f;             // 2^-6 (1 + 2^-6)
constexpr float kL2EpsSum = 6.103515625e-05f;             // 2^-14

// the bf16 image (its 16 bits) of a finite f32: round to nearest, ties to even
TOD_HD uint16_t l2_bf16_rne(float x) {
  const uint32_t b = __builtin_bit_cast(uint32_t, x);
  return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}

// eps(q) from the f32 values of |q|^2 and Rmax^2
TOD_HD float l2_eps(float q_norm2, float rmax2) {
  const float nq = sqrtf(q_norm2), rmax = sqrtf(rmax2);
  return kL2EpsLead * nq * rmax + kL2EpsSum * (nq + rmax) * (nq + rmax);
}

}  // namespace tod
