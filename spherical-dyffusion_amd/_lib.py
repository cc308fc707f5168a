"""ctypes binding of libsdy_amd.so (the C ABI declared in include/sdy_amd.h).

The HIP library is the product: there is NO Python/PyTorch fallback for any op.  If the shared object is
missing the import fails loudly (build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C spherical-dyffusion_amd/csrc`).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SDY_AMD_LIB: another build of the same library (A/B measurements of compile-time kernel switches, csrc/Makefile); never a fallback
LIB_PATH = os.environ.get("SDY_AMD_LIB") or os.path.join(_HERE, "libsdy_amd.so")

SDY_GRID = {"equiangular": 0, "legendre-gauss": 1}


class SdyError(RuntimeError):
    pass


class SdyConvArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x_bstride", C.c_long),
        ("wt", C.c_void_p), ("ldw", C.c_int),
        ("out", C.c_void_p), ("out_bstride", C.c_long),
        ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("HW", C.c_int),
        ("pa", C.c_void_p), ("pd", C.c_void_p),
        ("bias", C.c_void_p),
        ("add", C.c_void_p), ("add_bstride", C.c_long),
        ("add_mode", C.c_int),
        ("act", C.c_int),
        ("drop_p", C.c_float),
        ("keep_mask", C.c_void_p),
        ("seed", C.c_uint64), ("call", C.c_uint32), ("stream_id", C.c_uint32), ("batch_offset", C.c_uint32),
        ("rows_per_call", C.c_int),
        ("batch_scale", C.c_void_p),
        ("kernel_tag", C.c_int),
        ("w_h3", C.c_void_p),
        ("w_h3_scale", C.c_float),
        ("w_frag", C.c_void_p),
        ("w_frag_scale", C.c_float),
        ("stats", C.c_void_p),
        ("out_tiled", C.c_int),
        ("x_rows", C.c_void_p),
    ]


class SdyMlpArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x_bstride", C.c_long),
        ("pa", C.c_void_p), ("pd", C.c_void_p),
        ("w", C.c_void_p), ("w1_scale", C.c_float), ("w2_scale", C.c_float),
        ("b1", C.c_void_p), ("b2", C.c_void_p),
        ("out", C.c_void_p), ("out_bstride", C.c_long),
        ("add", C.c_void_p), ("add_bstride", C.c_long),
        ("add_a", C.c_void_p), ("add_d", C.c_void_p),
        ("B", C.c_int), ("E", C.c_int), ("hidden", C.c_int), ("HW", C.c_int),
        ("drop_p", C.c_float),
        ("seed", C.c_uint64), ("call", C.c_uint32), ("stream_fc1", C.c_uint32), ("stream_fc2", C.c_uint32),
        ("batch_offset", C.c_uint32),
        ("rows_per_call", C.c_int),
        ("batch_scale", C.c_void_p),
        ("stats", C.c_void_p),
        ("x_tiled", C.c_int),
        ("keep_hidden", C.c_void_p), ("keep_out", C.c_void_p),
        ("out_rows", C.c_void_p),
        ("add_by_launch_row", C.c_int),
    ]


class SdyPairArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x_bstride", C.c_long),
        ("w", C.c_void_p), ("w1_scale", C.c_float), ("w2_scale", C.c_float),
        ("b1", C.c_void_p),
        ("out", C.c_void_p), ("out_bstride", C.c_long),
        ("add", C.c_void_p), ("add_bstride", C.c_long),
        ("B", C.c_int), ("Cin", C.c_int), ("hidden", C.c_int), ("Cout", C.c_int), ("HW", C.c_int),
        ("stats", C.c_void_p),
    ]


SDY_MAX_VARS = 96


class SdyVarTable(C.Structure):
    _fields_ = [("nvars", C.c_int), ("data", C.c_void_p * SDY_MAX_VARS), ("mean", C.c_float * SDY_MAX_VARS),
                ("std", C.c_float * SDY_MAX_VARS)]


class SdyStepFinishArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("HW", C.c_int), ("T1", C.c_int), ("t", C.c_int),
        ("gen", C.c_void_p), ("n_out", C.c_int),
        ("prev_in", C.c_void_p), ("next_in", C.c_void_p), ("n_in", C.c_int),
        ("n_entries", C.c_int),
        ("out_idx", C.c_int * SDY_MAX_VARS), ("in_idx", C.c_int * SDY_MAX_VARS),
        ("gen_norm_tl", C.c_void_p * SDY_MAX_VARS), ("gen_tl", C.c_void_p * SDY_MAX_VARS),
        ("mean", C.c_float * SDY_MAX_VARS), ("std", C.c_float * SDY_MAX_VARS),
        ("presc_entry", C.c_int),
        ("presc_target", C.c_void_p), ("presc_mask", C.c_void_p),
        ("mask_value", C.c_int), ("interpolate", C.c_int),
        ("ar_init", C.c_void_p),
    ]


class SdySfnoConfig(C.Structure):
    _fields_ = [
        ("nlat", C.c_int), ("nlon", C.c_int),
        ("in_chans", C.c_int), ("out_chans", C.c_int),
        ("embed_dim", C.c_int), ("num_layers", C.c_int), ("mlp_hidden", C.c_int),
        ("lmax", C.c_int), ("mmax", C.c_int),
        ("data_grid", C.c_int),
        ("with_time_emb", C.c_int), ("time_dim", C.c_int),
        ("dropout_mlp", C.c_float), ("drop_path_rate", C.c_float),
        ("big_skip", C.c_int), ("pos_embed", C.c_int),
        ("gemm_mode", C.c_int),
    ]


class SdySfnoFwdArgs(C.Structure):
    _fields_ = [
        ("in_", C.c_void_p * 3), ("in_chans", C.c_int * 3),
        ("time", C.c_void_p),
        ("out", C.c_void_p),
        ("B", C.c_int),
        ("enable_dropout", C.c_int),
        ("seed", C.c_uint64), ("call", C.c_uint32), ("batch_offset", C.c_uint32),
        ("rows_per_call", C.c_int),
        ("keep_masks", C.POINTER(C.c_void_p)),
        ("drop_path_keep", C.c_void_p),
        ("ws", C.c_void_p), ("ws_floats", C.c_size_t),
        ("reuse_encoder", C.c_int),
        ("shared_inputs", C.c_int),
        ("gen_src", C.c_void_p), ("gen_chans", C.c_int), ("gen_pos", C.c_int),
        ("gen_coef", C.c_void_p), ("gen_noise", C.c_void_p),
    ]


SDY_DERIVED_MAX_LEVELS = 16


class SdyDerivedArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p * SDY_DERIVED_MAX_LEVELS), ("ps", C.c_void_p),
        ("lhf", C.c_void_p), ("prate", C.c_void_p), ("adv", C.c_void_p),
        ("s0", C.c_long), ("s1", C.c_long),
        ("n0", C.c_int), ("n1", C.c_int), ("T", C.c_int), ("HW", C.c_int), ("K", C.c_int),
        ("ak", C.c_float * (SDY_DERIVED_MAX_LEVELS + 1)), ("bk", C.c_float * (SDY_DERIVED_MAX_LEVELS + 1)),
        ("dry", C.c_void_p), ("twp", C.c_void_p), ("resid", C.c_void_p),
    ]


SDY_CORRECTOR_DRY_AIR = 1
SDY_CORRECTOR_ZERO_ADV = 2
SDY_CORRECTOR_BUDGET = {None: 0, "precipitation": 1, "evaporation": 2, "advection_and_precipitation": 3,
                        "advection_and_evaporation": 4}


class SdyCorrectorVar(C.Structure):
    _fields_ = [("base", C.c_void_p), ("stride", C.c_long), ("channel", C.c_int), ("mean", C.c_float), ("std", C.c_float)]


class SdyCorrectorOut(C.Structure):
    _fields_ = [("base", C.c_void_p), ("stride", C.c_long), ("channel", C.c_int)]


class SdyCorrectorArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("HW", C.c_int), ("K", C.c_int), ("flags", C.c_int), ("budget", C.c_int),
        ("ak", C.c_float * (SDY_DERIVED_MAX_LEVELS + 1)), ("bk", C.c_float * (SDY_DERIVED_MAX_LEVELS + 1)),
        ("area", C.c_void_p),
        ("gen_q", SdyCorrectorVar * SDY_DERIVED_MAX_LEVELS), ("in_q", SdyCorrectorVar * SDY_DERIVED_MAX_LEVELS),
        ("gen_ps", SdyCorrectorVar), ("in_ps", SdyCorrectorVar), ("gen_lhf", SdyCorrectorVar),
        ("gen_prate", SdyCorrectorVar), ("gen_adv", SdyCorrectorVar),
        ("out_ps", SdyCorrectorOut), ("out_lhf", SdyCorrectorOut), ("out_prate", SdyCorrectorOut),
        ("out_adv", SdyCorrectorOut),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


class SdyDryAirVar(C.Structure):
    _fields_ = [("base", C.c_void_p), ("stride_b", C.c_long), ("stride_t", C.c_long), ("channel", C.c_int),
                ("mean", C.c_float), ("std", C.c_float)]


class SdyDryAirArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("T", C.c_int), ("HW", C.c_int), ("K", C.c_int), ("accumulate", C.c_int),
        ("ak", C.c_float * (SDY_DERIVED_MAX_LEVELS + 1)), ("bk", C.c_float * (SDY_DERIVED_MAX_LEVELS + 1)),
        ("area", C.c_void_p),
        ("q", SdyDryAirVar * SDY_DERIVED_MAX_LEVELS), ("ps", SdyDryAirVar),
        ("gm", C.c_void_p), ("absdiff", C.c_void_p), ("mean_absdiff", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


SDY_HIST_MAX_BINS = 2048
SDY_HIST_FLAG_RANGE = 1


class SdyHistArgs(C.Structure):
    _fields_ = [
        ("nvars", C.c_int), ("data", C.c_void_p * SDY_MAX_VARS),
        ("s0", C.c_long * SDY_MAX_VARS), ("s1", C.c_long * SDY_MAX_VARS),
        ("n0", C.c_int), ("n1", C.c_int), ("T", C.c_int), ("HW", C.c_int),
        ("t_start", C.c_int), ("n_times", C.c_int), ("n_bins", C.c_int),
        ("state", C.c_void_p), ("counts", C.c_void_p),
    ]


class SdyCoarsenArgs(C.Structure):
    _fields_ = [
        ("nvars", C.c_int), ("data", C.c_void_p * SDY_MAX_VARS),
        ("s0", C.c_long * SDY_MAX_VARS), ("s1", C.c_long * SDY_MAX_VARS),
        ("out", C.c_void_p * SDY_MAX_VARS),
        ("n0", C.c_int), ("n1", C.c_int), ("T", C.c_int), ("HW", C.c_int),
        ("t_first", C.c_int), ("factor", C.c_int),
    ]


class SdyWindow(C.Structure):
    """sdy_window: embedded as `win` at the head of the structures below that read a window in place (filled by `windows.fill_window`); its fields
    also read and write as the embedding structure's own (`a.T` is `a.win.T`)."""
    _fields_ = [
        ("nvars", C.c_int), ("gen", C.c_void_p * SDY_MAX_VARS), ("target", C.c_void_p * SDY_MAX_VARS),
        ("gs0", C.c_long), ("gs1", C.c_long), ("ts1", C.c_long),
        ("n0", C.c_int), ("n1", C.c_int), ("T", C.c_int),
    ]


class SdyLeadSlots(C.Structure):
    """sdy_lead_slots: embedded as `slots` in the structures below that keep one accumulator slot per lead time (filled by
    `windows.fill_slots`); its fields also read and write as the embedding structure's own."""
    _fields_ = [("t0", C.c_int), ("t_start", C.c_int), ("n_slots", C.c_int), ("pool_times", C.c_int)]


class SdyVideoArgs(C.Structure):
    _anonymous_ = ("win",)
    _fields_ = [
        ("win", SdyWindow), ("HW", C.c_int),
        ("t_start", C.c_int), ("n_timesteps", C.c_int),
        ("gen_mean", C.c_void_p), ("target_mean", C.c_void_p), ("gen_sq", C.c_void_p), ("target_sq", C.c_void_p),
        ("err_var", C.c_void_p), ("err_min", C.c_void_p), ("err_max", C.c_void_p),
    ]


class SdyZonalArgs(C.Structure):
    _anonymous_ = ("win",)
    _fields_ = [
        ("win", SdyWindow), ("H", C.c_int), ("W", C.c_int),
        ("t_start", C.c_int), ("n_timesteps", C.c_int),
        ("gen_acc", C.c_void_p), ("target_acc", C.c_void_p),
    ]


class SdyMemberSumArgs(C.Structure):
    _anonymous_ = ("win",)
    _fields_ = [
        ("win", SdyWindow), ("HW", C.c_int),
        ("t0", C.c_int),
        ("gen_sum", C.c_void_p), ("target_sum", C.c_void_p),
    ]


SDY_MEMBER_STATS_MAX_MEMBERS = 64


class SdyMemberStatsArgs(C.Structure):
    _fields_ = [
        ("nvars", C.c_int), ("M", C.c_int), ("n1", C.c_int), ("HW", C.c_int),
        ("gen_sum", C.c_void_p), ("target_sum", C.c_void_p), ("weights", C.c_void_p),
        ("n_times", C.c_double),
        ("out", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


class SdyCoefRows(C.Structure):
    """sdy_coef_rows: embedded as `rows` in the two spectrum structures below (filled by `spectrum._fill_rows`); its fields also
    read and write as the embedding structure's own (`a.lmax` is `a.rows.lmax`)."""
    _fields_ = [
        ("gen_scale", C.c_void_p), ("target_scale", C.c_void_p),
        ("lmax", C.c_int), ("mtr", C.c_int),
        ("gen_fields", C.c_int), ("target_fields", C.c_int),
        ("gen_var_stride", C.c_int), ("gen_time_stride", C.c_int),
        ("target_var_stride", C.c_int), ("target_time_stride", C.c_int),
        ("nvars", C.c_int), ("n0", C.c_int), ("n1", C.c_int), ("T", C.c_int),
        ("t_start", C.c_int), ("n_timesteps", C.c_int),
    ]


class SdySpectrumArgs(C.Structure):
    _anonymous_ = ("rows",)
    _fields_ = [
        ("gen", C.c_void_p), ("target", C.c_void_p),
        ("rows", SdyCoefRows),
        ("gen_power", C.c_void_p), ("target_power", C.c_void_p), ("err_power", C.c_void_p),
    ]


class _SizedStructure(C.Structure):
    """An argument structure that carries its own size (`struct_size`, filled in here) and is therefore not part of
    `ABI_STRUCTS`: the library refuses a structure of another size at every call."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(type(self))


class SdyVectorSpectrumArgs(_SizedStructure):
    """`sdy_vector_spectrum_args`."""
    _anonymous_ = ("rows",)
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("gen_d", C.c_void_p), ("gen_m", C.c_void_p), ("target_d", C.c_void_p), ("target_m", C.c_void_p),
        ("rows", SdyCoefRows),
        ("gen_v_offset", C.c_int), ("target_v_offset", C.c_int),
        ("gen_rot", C.c_void_p), ("gen_div", C.c_void_p), ("target_rot", C.c_void_p), ("target_div", C.c_void_p),
        ("err_rot", C.c_void_p), ("err_div", C.c_void_p),
    ]


class SdyHelmholtzArgs(_SizedStructure):
    """`sdy_helmholtz_args`."""
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("Cs_d", C.c_void_p), ("Cs_m", C.c_void_p),
        ("scale", C.c_void_p),
        ("factor", C.c_void_p),
        ("out", C.c_void_p),
        ("lmax", C.c_int), ("mtr", C.c_int),
        ("fields", C.c_int), ("u_offset", C.c_int), ("v_offset", C.c_int), ("n_winds", C.c_int),
        ("out_fields", C.c_int), ("out_stride", C.c_int), ("n_out", C.c_int),
        ("part", C.c_int * 4),
    ]


class SdyVariabilityArgs(C.Structure):
    _anonymous_ = ("win",)
    _fields_ = [
        ("win", SdyWindow), ("HW", C.c_int),
        ("t0", C.c_int),
        ("first", C.c_int),
        ("s1", C.c_void_p), ("s2", C.c_void_p), ("p", C.c_void_p),
        ("origin_last", C.c_void_p),
    ]


class SdyVariabilityMapsArgs(C.Structure):
    _fields_ = [
        ("n_elems", C.c_long),
        ("s1", C.c_void_p), ("s2", C.c_void_p), ("p", C.c_void_p),
        ("origin_last", C.c_void_p),
        ("n_times", C.c_double),
        ("variance", C.c_void_p), ("lag1", C.c_void_p),
    ]


SDY_TV_SLOTS = 6


class SdyVariabilityStatsArgs(C.Structure):
    _fields_ = [
        ("nvars", C.c_int), ("M", C.c_int), ("n1", C.c_int), ("HW", C.c_int),
        ("s1", C.c_void_p), ("s2", C.c_void_p), ("p", C.c_void_p),
        ("origin_last", C.c_void_p), ("weights", C.c_void_p),
        ("n_times", C.c_double),
        ("out", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


SDY_REGION_MAX = 16
SDY_REGION_MAX_MEMBERS = 64


class SdyRegionSeriesArgs(C.Structure):
    _anonymous_ = ("win",)
    _fields_ = [
        ("win", SdyWindow), ("HW", C.c_int),
        ("n_regions", C.c_int),
        ("weights", C.c_void_p),
        ("out", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


SDY_EVENT_MAX = 8
SDY_EVENT_MAX_MEMBERS = 64


class SdyEventThresholds(C.Structure):
    """sdy_event_thresholds: embedded as `thr` in the structures below that test values against the events of the variables
    (filled by `EventAccumulator._fill`); its fields also read and write as the embedding structure's own."""
    _fields_ = [
        ("n_events", C.c_int),
        ("n_maps", C.c_int),
        ("below", C.c_ubyte * SDY_MAX_VARS), ("is_map", C.c_ubyte * SDY_MAX_VARS),
        ("map_first", C.c_int * SDY_MAX_VARS),
        ("scalars", C.c_void_p), ("maps", C.c_void_p),
    ]


class SdyEventArgs(C.Structure):
    _anonymous_ = ("win", "slots", "thr")
    _fields_ = [
        ("win", SdyWindow), ("H", C.c_int), ("W", C.c_int),
        ("slots", SdyLeadSlots),
        ("thr", SdyEventThresholds),
        ("acc", C.c_void_p),
    ]


SDY_FSS_MAX_RADII = 4


class SdyFssArgs(C.Structure):
    _anonymous_ = ("win", "slots", "thr")
    _fields_ = [
        ("win", SdyWindow), ("H", C.c_int), ("W", C.c_int),
        ("slots", SdyLeadSlots),
        ("thr", SdyEventThresholds),
        ("n_radii", C.c_int), ("radii", C.c_int * SDY_FSS_MAX_RADII),
        ("acc", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


SDY_SPELL_BINS = 16


class SdyEventSpellArgs(_SizedStructure):
    """`sdy_event_spell_args`: the window and the thresholds of `SdyEventArgs`, no slots, then the state and the duration
    histograms."""
    _anonymous_ = ("win", "thr")
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("win", SdyWindow), ("H", C.c_int), ("W", C.c_int),
        ("t0", C.c_int),
        ("thr", SdyEventThresholds),
        ("state", C.c_void_p), ("durations", C.c_void_p),
    ]


SDY_MAX_QUANTILES = 8


class SdyTimeQuantileAppendArgs(_SizedStructure):
    """`sdy_time_quantile_append_args`: one window into the series of sortable keys."""
    _anonymous_ = ("win",)
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("win", SdyWindow), ("H", C.c_int), ("W", C.c_int),
        ("t0", C.c_int), ("slot0", C.c_int), ("capacity", C.c_int), ("store_gen", C.c_int),
        ("series", C.c_void_p),
    ]


class SdyTimeQuantileSelectArgs(_SizedStructure):
    """`sdy_time_quantile_select_args`: quantiles of groups of trajectories of one variable block of a series."""
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("series", C.c_void_p), ("plane", C.c_long),
        ("n_traj", C.c_int), ("capacity", C.c_int), ("n_slots", C.c_int),
        ("first", C.c_int), ("step", C.c_int), ("count", C.c_int), ("stride", C.c_int), ("n_groups", C.c_int),
        ("nq", C.c_int), ("method", C.c_int),
        ("q", C.c_double * SDY_MAX_QUANTILES),
        ("out", C.c_void_p), ("valid", C.c_void_p),
    ]


SDY_ST_MAX_PAIRS = 128
SDY_ST_MAX_LON = 4096
SDY_ST_MAX_SEGMENT = 1024


class SdySpacetimeAppendArgs(_SizedStructure):
    """`sdy_spacetime_append_args`: the band rows of one window into the ring of zonal Fourier coefficients."""
    _anonymous_ = ("win",)
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("win", SdyWindow), ("H", C.c_int), ("W", C.c_int),
        ("R", C.c_int), ("north", C.c_int * SDY_ST_MAX_PAIRS), ("south", C.c_int * SDY_ST_MAX_PAIRS),
        ("K", C.c_int),
        ("lon_table", C.c_void_p),
        ("t0", C.c_int), ("t1", C.c_int),
        ("n_first", C.c_long),
        ("N", C.c_int),
        ("coef", C.c_void_p),
    ]


class SdySpacetimeSegmentPowerArgs(_SizedStructure):
    """`sdy_spacetime_segment_power_args`: one segment of the ring into the power accumulators."""
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("coef", C.c_void_p),
        ("nvars", C.c_int), ("M", C.c_int), ("B", C.c_int),
        ("N", C.c_int), ("R", C.c_int), ("K", C.c_int),
        ("first_slot", C.c_int), ("detrend", C.c_int),
        ("taper", C.c_void_p), ("time_table", C.c_void_p),
        ("acc", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


SDY_TC_MAX_K = 4
SDY_TC_MAX_GROUPS = 32
SDY_TC_SLOTS = 6


class SdyTimeCovarianceArgs(_SizedStructure):
    """`sdy_time_covariance_args`: one window into the state of the groups of one K."""
    _anonymous_ = ("win",)
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("win", SdyWindow), ("HW", C.c_int),
        ("t0", C.c_int),
        ("first", C.c_int),
        ("K", C.c_int), ("n_groups", C.c_int),
        ("members", (C.c_int * SDY_TC_MAX_K) * SDY_TC_MAX_GROUPS),
        ("sums", C.c_void_p), ("products", C.c_void_p), ("origins", C.c_void_p),
    ]


class SdyTimeCovarianceMapsArgs(_SizedStructure):
    """`sdy_time_covariance_maps_args`: covariance and correlation of one pair of one group."""
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("sums", C.c_void_p), ("products", C.c_void_p),
        ("K", C.c_int), ("i", C.c_int), ("j", C.c_int),
        ("n_elems", C.c_long),
        ("n_times", C.c_double),
        ("cov", C.c_void_p), ("corr", C.c_void_p),
    ]


class SdyTimeCovarianceStatsArgs(_SizedStructure):
    """`sdy_time_covariance_stats_args`: the weighted sums of every pair of the groups of one K."""
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("K", C.c_int), ("n_groups", C.c_int),
        ("M", C.c_int), ("n1", C.c_int), ("HW", C.c_int),
        ("sums", C.c_void_p), ("products", C.c_void_p), ("weights", C.c_void_p),
        ("n_times", C.c_double),
        ("out", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


SDY_BIN_MAX_TIMES = 64


class SdyBinnedSumArgs(_SizedStructure):
    """`sdy_binned_sum_args`: the counted times of one window, grouped by bin, into the bins' sums and extremes."""
    _anonymous_ = ("win",)
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("win", SdyWindow), ("HW", C.c_int),
        ("n_bins", C.c_int), ("bin_vars", C.c_int),
        ("pool_members", C.c_int),
        ("n_groups", C.c_int),
        ("group_bin", C.c_int * SDY_BIN_MAX_TIMES),
        ("group_end", C.c_ushort * SDY_BIN_MAX_TIMES),
        ("times", C.c_ushort * SDY_BIN_MAX_TIMES),
        ("gen_sum", C.c_void_p), ("target_sum", C.c_void_p),
        ("gen_max", C.c_void_p), ("gen_min", C.c_void_p), ("target_max", C.c_void_p), ("target_min", C.c_void_p),
    ]


SDY_GRAM_MAX_MEMBERS = 64


class SdyMemberGramArgs(C.Structure):
    _anonymous_ = ("win",)
    _fields_ = [
        ("win", SdyWindow), ("HW", C.c_int),
        ("weights", C.c_void_p),
        ("climatology", C.c_void_p * SDY_MAX_VARS),
        ("out", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
    ]


SDY_RANK_HIST_MAX_MEMBERS = 64


class SdyRankHistArgs(C.Structure):
    _anonymous_ = ("win", "slots")
    _fields_ = [
        ("win", SdyWindow), ("H", C.c_int), ("W", C.c_int),
        ("slots", SdyLeadSlots),
        ("counts", C.c_void_p), ("ties", C.c_void_p),
    ]


# every argument structure of include/sdy_amd.h, in header order: what sdy_abi_check compares
ABI_STRUCTS = (SdyConvArgs, SdyMlpArgs, SdyPairArgs, SdySfnoConfig, SdySfnoFwdArgs, SdyVarTable, SdyStepFinishArgs,
               SdyDerivedArgs, SdyCorrectorArgs, SdyDryAirArgs, SdyHistArgs, SdyCoarsenArgs, SdyVideoArgs, SdyZonalArgs,
               SdyMemberSumArgs, SdyMemberStatsArgs, SdySpectrumArgs, SdyVariabilityArgs, SdyVariabilityMapsArgs,
               SdyVariabilityStatsArgs, SdyRegionSeriesArgs, SdyEventArgs, SdyFssArgs, SdyMemberGramArgs,
               SdyRankHistArgs)

# name -> (restype, argtypes); every symbol include/sdy_amd.h declares
SIGNATURES = {
    "sdy_version": (C.c_int, []),
    "sdy_error_string": (C.c_char_p, [C.c_int]),
    "sdy_abi_check": (C.c_int, [C.POINTER(C.c_size_t), C.c_int]),
    "sdy_abi_sizes": (C.c_int, [C.POINTER(C.c_size_t), C.c_int]),
    "sdy_sht_tables_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdy_sht_plan_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sdy_sht_plan_create_ex": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sdy_sht_plan_destroy": (None, [C.c_void_p]),
    "sdy_sht_plan_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int * 6)]),
    "sdy_sht_plan_kernels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int * 2)]),
    "sdy_sht_workspace_floats": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "sdy_sht_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdy_sht_inverse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdy_rfft_lon": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sdy_legendre_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sdy_legendre_inv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sdy_irfft_lon": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sdy_irfft_lon_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p]),
    "sdy_instnorm_from_partials": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdy_gelu_stats": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p]),
    "sdy_affine_copy_stats": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sdy_dhconv_pack_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sdy_dhconv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sdy_dhconv_h3_pack_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sdy_dhconv_h3_pack_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "sdy_dhconv_h3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_void_p]),
    "sdy_dhconv_frag_supported": (C.c_int, [C.c_int, C.c_int]),
    "sdy_dhconv_frag_pack_bytes": (C.c_size_t, [C.c_int]),
    "sdy_dhconv_frag_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "sdy_dhconv_frag": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sdy_instnorm_coeffs": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdy_conv1x1": (C.c_int, [C.POINTER(SdyConvArgs), C.c_void_p]),
    "sdy_ensemble_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p]),
    "sdy_instnorm_from_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_long, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdy_mlp_h3_supported": (C.c_int, [C.c_int, C.c_int]),
    "sdy_mlp_h3_pack_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sdy_mlp_h3_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                  C.POINTER(C.c_float)]),
    "sdy_mlp_h3": (C.c_int, [C.POINTER(SdyMlpArgs), C.c_void_p]),
    "sdy_pair_h3_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "sdy_pair_h3_pack_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sdy_pair_h3_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                   C.POINTER(C.c_float)]),
    "sdy_pair_h3": (C.c_int, [C.POINTER(SdyPairArgs), C.c_void_p]),
    "sdy_conv256_h3_supported": (C.c_int, [C.c_int, C.c_int]),
    "sdy_conv256_h3_pack_bytes": (C.c_size_t, []),
    "sdy_conv256_h3_pack_bytes_cin": (C.c_size_t, [C.c_int]),
    "sdy_conv256_h3_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "sdy_conv256_h3_pack_cin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "sdy_h3_pack_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sdy_h3_pack_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "sdy_sfno_create": (C.c_int, [C.POINTER(SdySfnoConfig), C.POINTER(C.c_void_p)]),
    "sdy_sfno_destroy": (None, [C.c_void_p]),
    "sdy_sfno_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "sdy_sfno_ready": (C.c_int, [C.c_void_p]),
    "sdy_sfno_missing": (C.c_char_p, [C.c_void_p]),
    "sdy_sfno_workspace_floats": (C.c_size_t, [C.c_void_p, C.c_int]),
    "sdy_sfno_max_batch": (C.c_int, [C.c_void_p]),
    "sdy_sfno_forward": (C.c_int, [C.c_void_p, C.POINTER(SdySfnoFwdArgs), C.c_void_p]),
    "sdy_sfno_time_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdy_norm_pack": (C.c_int, [C.POINTER(SdyVarTable), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sdy_step_finish": (C.c_int, [C.POINTER(SdyStepFinishArgs), C.c_void_p]),
    "sdy_init_timeline": (C.c_int, [C.POINTER(SdyVarTable), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_void_p), C.c_void_p]),
    "sdy_lp_rel_terms": (C.c_int, [C.c_void_p, C.POINTER(SdyVarTable), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "sdy_cold_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdy_concat_channels": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p]),
    "sdy_time_mean_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int,
                                          C.c_float, C.c_void_p, C.c_void_p]),
    "sdy_status_flags": (C.c_int, [C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "sdy_status_flags_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "sdy_range_headroom_enable": (C.c_int, [C.c_int]),
    "sdy_range_headroom": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "sdy_dropout_stream_rounds": (C.c_int, []),
    "sdy_dropout_stream_words": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.POINTER(C.c_uint32)]),
    "sdy_cond_noise_fill": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "sdy_ensemble_series": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sdy_ensemble_series_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p,
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sdy_derived_water": (C.c_int, [C.POINTER(SdyDerivedArgs), C.c_void_p]),
    "sdy_corrector": (C.c_int, [C.POINTER(SdyCorrectorArgs), C.c_void_p]),
    "sdy_corrector_host": (C.c_int, [C.POINTER(SdyCorrectorArgs)]),
    "sdy_corrector_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sdy_dry_air_series": (C.c_int, [C.POINTER(SdyDryAirArgs), C.c_void_p]),
    "sdy_dry_air_series_host": (C.c_int, [C.POINTER(SdyDryAirArgs)]),
    "sdy_dry_air_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sdy_hist_add": (C.c_int, [C.POINTER(SdyHistArgs), C.c_void_p]),
    "sdy_hist_state_bytes": (C.c_size_t, [C.c_int]),
    "sdy_hist_state_unpack_host": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                             C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)]),
    "sdy_hist_plan_host": (C.c_int, [C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]),
    "sdy_hist_edges_host": (C.c_int, [C.c_float, C.c_float, C.c_int, C.c_void_p]),
    "sdy_hist_bins_host": (C.c_int, [C.c_void_p, C.c_long, C.c_float, C.c_float, C.c_int, C.c_void_p]),
    "sdy_time_coarsen": (C.c_int, [C.POINTER(SdyCoarsenArgs), C.c_void_p]),
    "sdy_time_coarsen_host": (C.c_int, [C.POINTER(SdyCoarsenArgs)]),
    "sdy_video_accumulate": (C.c_int, [C.POINTER(SdyVideoArgs), C.c_void_p]),
    "sdy_video_accumulate_host": (C.c_int, [C.POINTER(SdyVideoArgs)]),
    "sdy_zonal_accumulate": (C.c_int, [C.POINTER(SdyZonalArgs), C.c_void_p]),
    "sdy_zonal_accumulate_host": (C.c_int, [C.POINTER(SdyZonalArgs)]),
    "sdy_member_time_sum": (C.c_int, [C.POINTER(SdyMemberSumArgs), C.c_void_p]),
    "sdy_member_time_sum_host": (C.c_int, [C.POINTER(SdyMemberSumArgs)]),
    "sdy_member_map_stats": (C.c_int, [C.POINTER(SdyMemberStatsArgs), C.c_void_p]),
    "sdy_member_map_stats_host": (C.c_int, [C.POINTER(SdyMemberStatsArgs)]),
    "sdy_member_stats_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sdy_degree_power": (C.c_int, [C.POINTER(SdySpectrumArgs), C.c_void_p]),
    "sdy_degree_power_host": (C.c_int, [C.POINTER(SdySpectrumArgs)]),
    "sdy_vsht_tables_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sdy_vsht_plan_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "sdy_vsht_plan_destroy": (None, [C.c_void_p]),
    "sdy_vector_legendre_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sdy_vector_degree_power": (C.c_int, [C.POINTER(SdyVectorSpectrumArgs), C.c_void_p]),
    "sdy_vector_degree_power_host": (C.c_int, [C.POINTER(SdyVectorSpectrumArgs)]),
    "sdy_helmholtz_factors_host": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p]),
    "sdy_helmholtz_coefficients": (C.c_int, [C.POINTER(SdyHelmholtzArgs), C.c_void_p]),
    "sdy_helmholtz_coefficients_host": (C.c_int, [C.POINTER(SdyHelmholtzArgs)]),
    "sdy_time_variability_accumulate": (C.c_int, [C.POINTER(SdyVariabilityArgs), C.c_void_p]),
    "sdy_time_variability_accumulate_host": (C.c_int, [C.POINTER(SdyVariabilityArgs)]),
    "sdy_time_variability_maps": (C.c_int, [C.POINTER(SdyVariabilityMapsArgs), C.c_void_p]),
    "sdy_time_variability_maps_host": (C.c_int, [C.POINTER(SdyVariabilityMapsArgs)]),
    "sdy_time_variability_stats": (C.c_int, [C.POINTER(SdyVariabilityStatsArgs), C.c_void_p]),
    "sdy_time_variability_stats_host": (C.c_int, [C.POINTER(SdyVariabilityStatsArgs)]),
    "sdy_time_variability_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sdy_region_series": (C.c_int, [C.POINTER(SdyRegionSeriesArgs), C.c_void_p]),
    "sdy_region_series_host": (C.c_int, [C.POINTER(SdyRegionSeriesArgs)]),
    "sdy_region_series_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sdy_event_table_accumulate": (C.c_int, [C.POINTER(SdyEventArgs), C.c_void_p]),
    "sdy_event_table_accumulate_host": (C.c_int, [C.POINTER(SdyEventArgs)]),
    "sdy_event_frequency_accumulate": (C.c_int, [C.POINTER(SdyEventArgs), C.c_void_p]),
    "sdy_event_frequency_accumulate_host": (C.c_int, [C.POINTER(SdyEventArgs)]),
    "sdy_event_spell_accumulate": (C.c_int, [C.POINTER(SdyEventSpellArgs), C.c_void_p]),
    "sdy_event_spell_accumulate_host": (C.c_int, [C.POINTER(SdyEventSpellArgs)]),
    "sdy_time_quantile_append": (C.c_int, [C.POINTER(SdyTimeQuantileAppendArgs), C.c_void_p]),
    "sdy_time_quantile_append_host": (C.c_int, [C.POINTER(SdyTimeQuantileAppendArgs)]),
    "sdy_time_quantile_select": (C.c_int, [C.POINTER(SdyTimeQuantileSelectArgs), C.c_void_p]),
    "sdy_time_quantile_select_host": (C.c_int, [C.POINTER(SdyTimeQuantileSelectArgs)]),
    "sdy_spacetime_append": (C.c_int, [C.POINTER(SdySpacetimeAppendArgs), C.c_void_p]),
    "sdy_spacetime_append_host": (C.c_int, [C.POINTER(SdySpacetimeAppendArgs)]),
    "sdy_spacetime_segment_power": (C.c_int, [C.POINTER(SdySpacetimeSegmentPowerArgs), C.c_void_p]),
    "sdy_spacetime_segment_power_host": (C.c_int, [C.POINTER(SdySpacetimeSegmentPowerArgs)]),
    "sdy_spacetime_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "sdy_time_covariance_accumulate": (C.c_int, [C.POINTER(SdyTimeCovarianceArgs), C.c_void_p]),
    "sdy_time_covariance_accumulate_host": (C.c_int, [C.POINTER(SdyTimeCovarianceArgs)]),
    "sdy_time_covariance_maps": (C.c_int, [C.POINTER(SdyTimeCovarianceMapsArgs), C.c_void_p]),
    "sdy_time_covariance_maps_host": (C.c_int, [C.POINTER(SdyTimeCovarianceMapsArgs)]),
    "sdy_time_covariance_stats": (C.c_int, [C.POINTER(SdyTimeCovarianceStatsArgs), C.c_void_p]),
    "sdy_time_covariance_stats_host": (C.c_int, [C.POINTER(SdyTimeCovarianceStatsArgs)]),
    "sdy_time_covariance_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sdy_binned_time_accumulate": (C.c_int, [C.POINTER(SdyBinnedSumArgs), C.c_void_p]),
    "sdy_binned_time_accumulate_host": (C.c_int, [C.POINTER(SdyBinnedSumArgs)]),
    "sdy_fss_accumulate": (C.c_int, [C.POINTER(SdyFssArgs), C.c_void_p]),
    "sdy_fss_accumulate_host": (C.c_int, [C.POINTER(SdyFssArgs)]),
    "sdy_fss_encode": (C.c_int, [C.POINTER(SdyFssArgs), C.c_void_p]),
    "sdy_fss_sum": (C.c_int, [C.POINTER(SdyFssArgs), C.c_void_p]),
    "sdy_fss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sdy_member_gram": (C.c_int, [C.POINTER(SdyMemberGramArgs), C.c_void_p]),
    "sdy_member_gram_host": (C.c_int, [C.POINTER(SdyMemberGramArgs)]),
    "sdy_member_gram_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sdy_rank_hist_accumulate": (C.c_int, [C.POINTER(SdyRankHistArgs), C.c_void_p]),
    "sdy_rank_hist_accumulate_host": (C.c_int, [C.POINTER(SdyRankHistArgs)]),
    "sdy_profile_enable": (C.c_int, [C.c_int]),
    "sdy_profile_stage_count": (C.c_int, []),
    "sdy_profile_stage_name": (C.c_char_p, [C.c_int]),
    "sdy_profile_read": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_long), C.c_int]),
    "sdy_profile_read_rows": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_long), C.c_int]),
    "sdy_relay_pool_create": (C.c_int, [C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_ubyte)]),
    "sdy_relay_pool_destroy": (C.c_int, [C.c_void_p]),
    "sdy_ipc_open": (C.c_int, [C.POINTER(C.c_ubyte), C.POINTER(C.c_void_p)]),
    "sdy_ipc_close": (C.c_int, [C.c_void_p]),
    "sdy_copy_nocu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}


def _load():
    # torch first: PyTorch-ROCm ships its own libamdhip64, and the process must end up with ONE HIP runtime.  Loaded after
    # torch, libsdy_amd.so binds to the runtime torch already brought in (same soname); loaded BEFORE it, the library pulls
    # /opt/rocm's copy, torch adds its own, and every sdy_* call then fails with "no ROCm-capable device is detected"
    # (seen on the GPU box with `import sdy_amd` ahead of `import torch`).
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP library is required (no CPU/PyTorch fallback exists). "
            "Build it with `make -C spherical-dyffusion_amd/csrc` or `__graft_entry__.build()`."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    # the argument structures carry no size field: the bindings' layouts must be the library's (include/sdy_amd.h, sdy_abi_check)
    ours = (C.c_size_t * len(ABI_STRUCTS))(*[C.sizeof(t) for t in ABI_STRUCTS])
    if lib.sdy_abi_check(ours, len(ours)) != 0:
        theirs = (C.c_size_t * len(ours))()
        theirs = list(theirs) if lib.sdy_abi_sizes(theirs, len(theirs)) == 0 else "another number of structures"
        raise ImportError(f"{LIB_PATH}: argument structures of the bindings and of the library differ: "
                          f"{[t.__name__ for t in ABI_STRUCTS]} are {list(ours)} bytes in the bindings and {theirs} in the "
                          "library: rebuild the library (make -C spherical-dyffusion_amd/csrc)")
    return lib


lib = _load()


def default_gemm_mode() -> str:
    """"h3" (split-fp16 3-pass MFMA, the default) or "f32" (fp32-input MFMA); both hold the same parity tolerances."""
    m = os.environ.get("SDY_GEMM_MODE", "h3")
    if m not in ("h3", "f32"):
        raise ValueError(f"SDY_GEMM_MODE must be 'h3' or 'f32', got {m!r}")
    return m


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib.sdy_error_string(rc).decode()
        raise SdyError(f"{what or 'sdy call'} failed with code {rc}: {msg}")


def ptr(t) -> int:
    """Device/host pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


def aligned(t):
    """`t`, or a copy of it when its first element is not on a 16-byte boundary (None stays None).  `.contiguous()` returns a
    contiguous VIEW as it is, whatever its storage offset; the float4 kernels refuse such a pointer (SDY_ERR_ALIGN,
    include/sdy_amd.h).  A fresh allocation is aligned; a copy keeps the order of the axes."""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def current_stream() -> int:
    import torch

    return torch.cuda.current_stream().cuda_stream
