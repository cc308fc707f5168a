// What the kernels that test an ensemble's values against the thresholds of its events share (event_verif.hip, fss.hip,
// spells.hip): the per-thread registers of a variable's events, the signed thresholds of a unit of grid points, the count of
// the members in each event and the dispatch over event count and load width.  The event count is a template argument: every
// array here is indexed at compile time only and stays in registers.  The arithmetic of a point is events.h.
#pragma once
#include "common.h"
#include "events.h"
#include "window.h"

// independent member loads a thread issues before it consumes the first: with more than 4 events the thresholds and counters
// of a unit take the registers that the second half of 8 loads would
template <int EC>
constexpr int kInFlight = EC > 4 ? 4 : 8;

// What a thread keeps per event of variable v, set once before its first unit: the sign that folds the direction into the
// operands (sdy_ev_signed, events.h), the signed scalar threshold, and the plane of a map threshold.  All three are
// wave-uniform, and are moved to vector registers on purpose: with 8 events they, and the map planes' 64-bit bases, would
// take more scalar registers than a wave has, and vector registers are not what limits these kernels.
template <int EC>
struct EventRegs {
  unsigned sign[EC];
  float scalar[EC];
  int plane[EC];
};
template <int EC>
__device__ __forceinline__ void event_regs(const sdy_event_thresholds& a, int v, unsigned is_map, unsigned below, EventRegs<EC>& r) {
#pragma unroll
  for (int e = 0; e < EC; ++e) {
    r.sign[e] = sdy_ev_sign((below >> e) & 1u);
    r.scalar[e] = sdy_ev_signed(a.scalars[v * EC + e], r.sign[e]);
    r.plane[e] = sdy_ev_map_plane(a.map_first[v], is_map, e);
    asm volatile("" : "+v"(r.sign[e]), "+v"(r.scalar[e]), "+v"(r.plane[e]));
  }
}

// The signed thresholds of the W4 points from point `at` of a plane on, all EC events: a map event loads its row once per unit,
// a scalar event costs no load.  is_map is wave-uniform: the branch does not diverge.
template <int W4, int EC>
__device__ __forceinline__ void thresholds(const sdy_event_thresholds& a, unsigned is_map, const EventRegs<EC>& r, long plane, unsigned at,
                                           float (&c)[EC][W4]) {
  // (through a vector register and back: the EC bit tests are made here, once per unit, as scalar compares; hoisted out of
  // the kernel's loops they would be kept as EC lane masks in pairs of scalar registers)
  unsigned bits = is_map;
  asm volatile("" : "+v"(bits));
  bits = __builtin_amdgcn_readfirstlane(bits);
#pragma unroll
  for (int e = 0; e < EC; ++e) {
    if ((bits >> e) & 1u) {
      const Vec<W4> m = ld<W4>(a.maps + ((long)r.plane[e] * plane + at));
#pragma unroll
      for (int q = 0; q < W4; ++q) c[e][q] = sdy_ev_signed(comp(m, q), r.sign[e]);
    } else {
#pragma unroll
      for (int q = 0; q < W4; ++q) c[e][q] = r.scalar[e];
    }
  }
}

// k += (x > c), as the pair compare-into-VCC / add-with-carry and nothing else.  Written out because the compiler, left to
// itself, lines up the comparisons of a whole batch of members ahead of the additions -- one 64-bit lane mask in a pair of scalar
// registers each, up to 128 of them -- and spills scalar registers.  A NaN on either side compares false.
__device__ __forceinline__ void count_if_above(int& k, float x, float c) {
  asm("v_cmp_gt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(k) : "v"(x), "v"(c) : "vcc");
}

// k[e][q] += the members of the W4 points at byte offset off_b (of member 0's time) that are in event e, kInFlight loads in
// flight; c: the signed thresholds
template <int W4, int EC>
__device__ __forceinline__ void count_members(const float* g, long gs0, int M, unsigned off_b, const EventRegs<EC>& r,
                                              const float (&c)[EC][W4], int (&k)[EC][W4]) {
  constexpr int F = kInFlight<EC>;
  int i0 = 0;
  for (; i0 + F <= M; i0 += F) {
    Vec<W4> x[F];
#pragma unroll
    for (int j = 0; j < F; ++j) x[j] = ld_u<W4>(g + (long)(i0 + j) * gs0, off_b);
#pragma unroll
    for (int j = 0; j < F; ++j)
#pragma unroll
      for (int e = 0; e < EC; ++e)
#pragma unroll
        for (int q = 0; q < W4; ++q) count_if_above(k[e][q], sdy_ev_signed(comp(x[j], q), r.sign[e]), c[e][q]);
  }
  if (i0 < M) {
    Vec<W4> x[F - 1];
#pragma unroll
    for (int j = 0; j < F - 1; ++j)
      if (i0 + j < M) x[j] = ld_u<W4>(g + (long)(i0 + j) * gs0, off_b);
#pragma unroll
    for (int j = 0; j < F - 1; ++j)
      if (i0 + j < M) {
#pragma unroll
        for (int e = 0; e < EC; ++e)
#pragma unroll
          for (int q = 0; q < W4; ++q) count_if_above(k[e][q], sdy_ev_signed(comp(x[j], q), r.sign[e]), c[e][q]);
      }
  }
}

// Launch<4 or 1, E>::go(args...) for the run-time load width and event count E = 1 .. SDY_EVENT_MAX (the entry points' checks)
template <template <int, int> class Launch, class... Args>
void dispatch(bool vec, int E, Args... args) {
  switch (E) {
#define SDY_EV_CASE(N)                \
  case N:                             \
    if (vec)                          \
      Launch<4, N>::go(args...);      \
    else                              \
      Launch<1, N>::go(args...);      \
    break;
    SDY_EV_CASE(1) SDY_EV_CASE(2) SDY_EV_CASE(3) SDY_EV_CASE(4) SDY_EV_CASE(5) SDY_EV_CASE(6) SDY_EV_CASE(7) SDY_EV_CASE(8)
#undef SDY_EV_CASE
  }
}
