// What the entry points that embed an sdy_event_thresholds or an sdy_lead_slots (include/sdy_amd.h) share (rank_hist.hip,
// event_verif.hip, fss.hip, spells.hip): the checks of the two descriptors, for the device and the host entry points alike,
// the alignment test of the threshold maps, the threshold of a point as the _host twins read it, and the slot of a window
// time.  What the kernels do with the thresholds is event_count.h.
#pragma once
#include "common.h"
#include "events.h"

// everything of the slots that bounds an accumulator index; T: the times of the window
inline int sdy_lead_slots_check(const sdy_lead_slots* s, int T) {
  if (s->n_slots < 1 || s->t0 < 0 || s->t0 > T) return SDY_ERR_ARG;
  if (s->pool_times) {
    if (s->n_slots != 1) return SDY_ERR_ARG;
  } else if (s->t_start < 0 || (long)s->t_start + (long)T > (long)s->n_slots) {
    // window times t_start .. t_start + T - 1 must all exist (in 64 bits: no wrap)
    return SDY_ERR_ARG;
  }
  return SDY_OK;
}

// the slot of window time t (< n_slots: sdy_lead_slots_check).  By value: through a reference into a kernel's by-value
// arguments the compiler schedules rank_hist_kernel differently (one more vector register).
SDY_EV_HD long sdy_lead_slot(const sdy_lead_slots s, long t) { return s.pool_times ? 0 : (long)s.t_start + t; }

// everything of the thresholds that bounds an address, the SDY_ERR_ARG part
inline int sdy_event_thresholds_check(const sdy_event_thresholds* thr, int nvars) {
  if (!thr->scalars || ((uintptr_t)thr->scalars & 3)) return SDY_ERR_ARG;
  if (thr->n_events < 1 || thr->n_events > SDY_EVENT_MAX) return SDY_ERR_ARG;
  for (int v = 0; v < nvars; ++v) {
    const unsigned is_map = thr->is_map[v] & ((1u << thr->n_events) - 1u);
    if (!is_map) continue;
    if (!thr->maps || ((uintptr_t)thr->maps & 3) || thr->n_maps < 1 || thr->map_first[v] < 0 ||
        (long)thr->map_first[v] + __builtin_popcount(is_map) > (long)thr->n_maps)
      return SDY_ERR_ARG;
  }
  return SDY_OK;
}

// the SDY_ERR_UNSUPPORTED part, after sdy_event_thresholds_check: 64-bit flat indices into the maps; plane = H * W.  (Apart:
// fss.hip has argument checks of its own between the two.)
inline int sdy_event_thresholds_supported(const sdy_event_thresholds* thr, int nvars, long plane) {
  for (int v = 0; v < nvars; ++v)
    if ((thr->is_map[v] & ((1u << thr->n_events) - 1u)) && (long)thr->n_maps * plane >= (1L << 40)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

// 16-byte loads of the maps allowed?
inline bool sdy_event_thresholds_vec4(const sdy_event_thresholds* thr) { return ((uintptr_t)thr->maps & 15) == 0; }

// the threshold of event e of variable v at grid point p, host side
inline float sdy_event_threshold_host(const sdy_event_thresholds* thr, int v, int e, long plane, long p) {
  if ((thr->is_map[v] >> e) & 1u) return thr->maps[(long)sdy_ev_map_plane(thr->map_first[v], thr->is_map[v], e) * plane + p];
  return thr->scalars[v * thr->n_events + e];
}
