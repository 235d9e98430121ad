// Device helpers of the stochastic-beam-search selection, shared by its two homes: sbs_select_f32_kernel
// (sbs.hip, a launch per char) and the selection inside gen_persist_sbs_kernel (gen_persist_sbs.hip, a whole
// call per launch).  Both translation units see the same text, so a value computed by one is the other's
// bit for bit.  (No product of two floats in here: nothing for the compiler to contract.)
#pragma once
#include <cmath>
#include "common.h"
#include "gen_sample.h"

namespace gk {

namespace {
// floats -> unsigned keys with the same order (-0 and +0 share a key); 0 is kept free for "no candidate"
DEV unsigned sbs_key(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  b = (b >> 31) ? ~b : (b | 0x80000000u);
  return b ? b : 1u;
}
DEV float sbs_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
DEV unsigned sbs_umax(unsigned u) {   // identical in every lane
  return ~(unsigned)wave_min_dpp((int)~(u ^ 0x80000000u)) ^ 0x80000000u;
}

// the truncated perturbed value of a child: g its own, Z its row's maximum, Gb the parent's
DEV float sbs_truncate(float Gb, float g, float Z) {
  const float d = g - Z;   // <= 0
  const float l1 = d == 0.f ? -INFINITY : (d > -0.6931f ? logf(-expm1f(d)) : log1pf(-expf(d)));
  const float v = (Gb - g) + l1;
  return (Gb - fmaxf(0.f, v)) - log1pf(expf(-fabsf(v)));
}
}  // namespace

}  // namespace gk
