// Spell durations of threshold events (consecutive dry days, warm spells), as ONE definition for the device kernel
// (spells.hip) and the host entry point sdy_event_spell_accumulate_host: the state of a trajectory, the step that advances
// it by one counted time, the bin of a duration, and where a state word and a histogram count live.  When a value is in an
// event is events.h.  Integers and comparisons only: nothing here rounds.
#pragma once
#include "../../include/sdy_amd.h"   // SDY_SPELL_BINS = 16 duration bins: edges 1, 2, 4, .., 16384
#include "events.h"

#define SDY_SPELL_WORDS 4  // 32-bit words of a state element, in this order:
#define SDY_SPELL_RUN 0     //   the length of the spell open after the last counted time (0: that time was outside the event)
#define SDY_SPELL_LONGEST 1 //   the maximum `run` has reached
#define SDY_SPELL_SPELLS 2  //   the spells begun
#define SDY_SPELL_HITS 3    //   the counted times in the event

// The bin of a duration d >= 1: the number of edges 1, 2, 4, .., 16384 that are < d, at most 15 -- d = 1 -> 0, 2 -> 1, 3..4 ->
// 2, 5..8 -> 3, .., 8193..16384 -> 14, anything longer -> 15.  That is the bit length of d - 1.
SDY_EV_HD int sdy_spell_bin(unsigned d) {
  if (d <= 1u) return 0;
  const int bits = 32 - __builtin_clz(d - 1u);
  return bits < SDY_SPELL_BINS - 1 ? bits : SDY_SPELL_BINS - 1;
}

// One counted time of a trajectory: `in` is 1 when its value is in the event, else 0.  -> the length of the spell that this time
// ends (the first time outside the event after it), 0 when it ends none.  A spell still open is in `run` only.  Written without
// a condition on `in`, so that the kernel keeps it as a 0 / 1 register and not as a lane mask per (event, point).
SDY_EV_HD unsigned sdy_spell_step(unsigned& run, unsigned& longest, unsigned& spells, unsigned& hits, unsigned in) {
  const unsigned keep = 0u - in;                   // all ones in the event, else 0
  const unsigned ended = run & ~keep;
  const unsigned open = run < 1u ? run : 1u;       // min(run, 1): 1 when a spell was open before this time
  spells += in & (open ^ 1u);
  run = (run + 1u) & keep;
  hits += in;
  longest = run > longest ? run : longest;
  return ended;
}

// The trajectories of a variable: rows 0 .. n0*n1 - 1 are the generated ones (member i0 = r / n1, sample i1 = r % n1), rows
// n0*n1 .. n0*n1 + n1 - 1 the targets (sample r - n0*n1): side 0 and side 1 of the histograms.
SDY_EV_HD long sdy_spell_rows(long n0, long n1) { return n0 * n1 + n1; }

// state[v, e, word, r, p] of the contiguous (nvars, E, 4, rows, plane) 32-bit words: four planes per (variable, event), so
// that the 4 points of a lane are one 16-byte access and the accesses of a wave are contiguous.  The entry points bound the
// product below 2^50.
SDY_EV_HD long sdy_spell_state_at(long v, long E, long e, long word, long rows, long r, long plane, long p) {
  return ((((v * E + e) * SDY_SPELL_WORDS + word) * rows + r) * plane) + p;
}

// durations[v, e, side, lat, bin] of the contiguous (nvars, E, 2, H, 16) float64 accumulator
SDY_EV_HD long sdy_spell_duration_at(long v, long E, long e, long side, long H, long lat, long bin) {
  return ((((v * E + e) * 2 + side) * H + lat) * SDY_SPELL_BINS) + bin;
}
