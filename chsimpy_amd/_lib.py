"""ctypes binding of ``libchs_hip.so`` (C ABI: ``include/chs_hip.h``).

The HIP library *is* the product path: there is no CPU fallback.  A missing
library, a missing symbol or a missing GPU is an error raised here, loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libchs_hip.so')

CHS_OK, CHS_EINVAL, CHS_EHIP, CHS_ENAN, CHS_ESTATE, CHS_ECHECK, CHS_ELIMIT = 0, -1, -2, -3, -4, -5, -6
CHS_F64, CHS_F32 = 0, 1
CHS_ENGINE_AUTO, CHS_ENGINE_DIRECT, CHS_ENGINE_FAST, CHS_ENGINE_CHIRP = 0, 1, 2, 3
CHS_CHIRP_AUTO_MIN_N = 129    # the smallest N that 'auto' gives to the chirp engine (include/chs_hip.h)
CHS_STOP_NONE, CHS_STOP_ENERGY, CHS_STOP_TIME_LIMIT = 0, 1, 2
CHS_STEP_CARRY_HAT = 1
CHS_STEP_REDERIVE_HAT = 2
CHS_STEP_LAST_CALL = 4
CHS_STEP_KEEP_T1 = 8
CHS_NKERNELS = 8
CHS_MORPH_WORDS = 7           # int64 words of chs_morphology: Q0, Q1, Q2, QD, Q3, Q4, border
CHS_CC_WORDS = 7              # int64 words of chs_components: count, area, largest, sumsq, inner, spanning, largest_first
CHS_CC_COLS = 6               # int32 columns of its table: first, area, imin, imax, jmin, jmax
CHS_CC_BELOW, CHS_CC_ABOVE = 0, 1
CHS_DT_WORDS = 5              # int64 words of chs_distance: fg, d2max, d2max_first, sumd2, ninf
CHS_DT_INF = 1 << 30          # D2 of every pixel of a grid without background
CHS_CH_WORDS = 24             # int64 words of chs_chords: six per (phase, direction)
CHS_CMP_IWORDS = 7            # int64 words of chs_composition: n_total, n_nan, n_inf, n_below, n_under, n_over, nbins
CHS_CMP_FWORDS = 11           # its float64 words: min, max, sum, sum_below, center, m2, m3, m4, lo, hi, scale
CHS_CMP_MAX_BINS = 4096
CHS_CMP_MAX_RANKS = 8         # ranks of one chs_composition_select
CHS_TP_WORDS = 8              # int64 words of chs_two_point: n, the four neighbour counts and the table's sum per phase
CHS_TP_MAX_R = 256            # rmax of chs_two_point at most
CHS_TP_CHUNK = 2048           # the pixels of a row that one workgroup of its pair kernel owns
CHS_CT_WORDS = 16             # int64 words of chs_contour (chsimpy_amd/contour.py names them)
CHS_CT_SUMS = 6               # its float64 sums: txx, txy, tyy, k1, ka, k2
CHS_CT_MAX_BINS = 1024        # bins of its curvature histogram at most
CHS_SH_WORDS = 17             # int64 words of chs_shapes (chsimpy_amd/shapes.py names them)
CHS_SH_COLS = 16              # int64 columns of its table
CHS_TR_WORDS = 25             # int64 words of chs_track (chsimpy_amd/tracking.py names them)
CHS_TH_WORDS = 7              # int64 words of chs_thickness: fg, t2max, nmax, sumt2, ninf, kept, work
CHS_TH_KEPT, CHS_TH_WORK = 5, 6
CHS_GEO_WORDS = 16            # int64 words of chs_geodesic (chsimpy_amd/geodesic.py names them)
CHS_GEO_ROUNDS, CHS_GEO_LIMIT = 14, 15
CHS_SK_WORDS = 17             # int64 words of chs_skeleton (chsimpy_amd/skeleton.py names them)
CHS_SK_SUBITERS, CHS_SK_LIMIT = 15, 16
CHS_TRN_WORDS = 10            # int64 words of chs_transport (chsimpy_amd/transport.py names them)
CHS_TRN_VALS = 8              # doubles of chs_transport
CHS_TRN_CC_COUNT, CHS_TRN_ITERS, CHS_TRN_LIMIT = 2, 7, 9

STOP_NAMES = {CHS_STOP_NONE: 'None', CHS_STOP_ENERGY: 'energy', CHS_STOP_TIME_LIMIT: 'time-limit'}
STOP_CODES = {v: k for k, v in STOP_NAMES.items()}
ENGINES = {'auto': CHS_ENGINE_AUTO, 'direct': CHS_ENGINE_DIRECT, 'fast': CHS_ENGINE_FAST, 'chirp': CHS_ENGINE_CHIRP}
DTYPES = {'float64': CHS_F64, 'f64': CHS_F64, 'float32': CHS_F32, 'f32': CHS_F32}

# every symbol include/chs_hip.h declares
SYMBOLS = (
    'chs_create', 'chs_destroy', 'chs_pool_clear', 'chs_pool_count', 'chs_set_U', 'chs_init_U_pcg64', 'chs_get_U', 'chs_prepare', 'chs_step_n',
    'chs_get_state', 'chs_set_state', 'chs_set_jitter_noise', 'chs_set_jitter_pcg64', 'chs_dctn', 'chs_get_mu', 'chs_test_math', 'chs_test_math_cols',
    'chs_engine', 'chs_kernel_name', 'chs_profile_steps', 'chs_last_step_ms',
    'chs_last_error', 'chs_version',
    'chs_batch_create', 'chs_batch_destroy', 'chs_batch_set_U', 'chs_batch_init_U_pcg64', 'chs_batch_get_U',
    'chs_batch_prepare', 'chs_batch_step_n', 'chs_batch_get_state', 'chs_batch_set_state',
    'chs_batch_step_n_queued', 'chs_batch_member_rows', 'chs_batch_engine',
    'chs_structure_factor_bins', 'chs_structure_factor', 'chs_structure_factor_last_ms', 'chs_batch_structure_factor',
    'chs_morphology', 'chs_morphology_last_ms', 'chs_batch_morphology',
    'chs_components', 'chs_components_table', 'chs_components_labels', 'chs_components_last_ms', 'chs_components_tile',
    'chs_batch_components', 'chs_batch_components_table', 'chs_batch_components_labels',
    'chs_distance_bins', 'chs_distance', 'chs_distance_hist', 'chs_distance_map', 'chs_distance_last_ms', 'chs_distance_tile',
    'chs_batch_distance', 'chs_batch_distance_hist', 'chs_batch_distance_map',
    'chs_chords_bins', 'chs_chords', 'chs_chords_hist', 'chs_chords_last_ms', 'chs_chords_tile',
    'chs_batch_chords', 'chs_batch_chords_hist',
    'chs_composition', 'chs_composition_hist', 'chs_composition_select', 'chs_composition_last_ms', 'chs_composition_tile',
    'chs_batch_composition', 'chs_batch_composition_hist', 'chs_batch_composition_select', 'chs_batch_composition_last_ms',
    'chs_two_point_max_r', 'chs_two_point_size', 'chs_two_point', 'chs_two_point_counts', 'chs_two_point_last_ms',
    'chs_two_point_tile', 'chs_batch_two_point', 'chs_batch_two_point_counts', 'chs_batch_two_point_last_ms',
    'chs_contour', 'chs_contour_hist', 'chs_contour_map', 'chs_contour_last_ms', 'chs_contour_tile',
    'chs_batch_contour', 'chs_batch_contour_hist', 'chs_batch_contour_map', 'chs_batch_contour_last_ms',
    'chs_shapes', 'chs_shapes_table', 'chs_shapes_last_ms', 'chs_batch_shapes', 'chs_batch_shapes_table',
    'chs_track', 'chs_track_pairs', 'chs_track_reset', 'chs_track_last_ms',
    'chs_batch_track', 'chs_batch_track_pairs', 'chs_batch_track_reset',
    'chs_thickness_work_default', 'chs_thickness_reach', 'chs_thickness', 'chs_thickness_hist', 'chs_thickness_map',
    'chs_thickness_last_ms', 'chs_batch_thickness', 'chs_batch_thickness_hist', 'chs_batch_thickness_map',
    'chs_batch_thickness_last_ms',
    'chs_geodesic_bins', 'chs_geodesic_rounds_default', 'chs_geodesic', 'chs_geodesic_hist', 'chs_geodesic_profile',
    'chs_geodesic_map', 'chs_geodesic_last_ms', 'chs_geodesic_relax_ms', 'chs_batch_geodesic', 'chs_batch_geodesic_hist',
    'chs_batch_geodesic_profile', 'chs_batch_geodesic_map', 'chs_batch_geodesic_last_ms',
    'chs_skeleton_subiters_default', 'chs_skeleton', 'chs_skeleton_hist', 'chs_skeleton_plane', 'chs_skeleton_last_ms',
    'chs_skeleton_thin_ms', 'chs_batch_skeleton', 'chs_batch_skeleton_hist', 'chs_batch_skeleton_plane',
    'chs_batch_skeleton_last_ms', 'chs_batch_skeleton_thin_ms',
    'chs_transport_iters_default', 'chs_transport', 'chs_transport_profile', 'chs_transport_map', 'chs_transport_last_ms',
    'chs_transport_solve_ms', 'chs_batch_transport', 'chs_batch_transport_profile', 'chs_batch_transport_map',
    'chs_batch_transport_last_ms', 'chs_batch_transport_solve_ms',
)

# the N a batch takes (include/chs_hip.h: chs_batch_create): the fast engine's batch at BATCH_SIZES, the chirp engine's
# at every other N in [BATCH_CHIRP_MIN_N, BATCH_CHIRP_MAX_N] (CHS_BATCH_CHIRP_MIN_N / _MAX_N) where the members run it
BATCH_SIZES = (128, 256, 512, 1024, 2048)
BATCH_CHIRP_MIN_N, BATCH_CHIRP_MAX_N = 8, 4096
FAST_SIZES = (128, 256, 512, 1024, 2048, 4096, 8192)   # the fast engine's N ('auto' resolves to it there)


class chs_consts(C.Structure):
    _fields_ = [('N', C.c_int32), ('dtype', C.c_int32), ('device', C.c_int32), ('engine', C.c_int32),
                ('adaptive_time', C.c_int32), ('full_sim', C.c_int32),
                ('RT', C.c_double), ('BRT', C.c_double), ('B', C.c_double), ('A0', C.c_double),
                ('A1', C.c_double), ('Amr', C.c_double), ('kappa_tilde', C.c_double), ('L', C.c_double),
                ('delx', C.c_double), ('delt', C.c_double), ('delt_max', C.c_double),
                ('M_tilde', C.c_double), ('threshold', C.c_double), ('time_limit_s', C.c_double)]


class chs_state(C.Structure):
    _fields_ = [('delt', C.c_double), ('time_delta_sum', C.c_double), ('time_passed', C.c_double),
                ('tau0', C.c_double), ('t0', C.c_double), ('computed_steps', C.c_int64),
                ('skip_check', C.c_int32), ('stop_reason', C.c_int32)]


class EngineError(RuntimeError):
    pass


class ThicknessLimitError(EngineError):
    """A thickness look that was refused (CHS_ELIMIT): it needs ``work`` disc pixels, the caller allowed ``limit``.  Nothing
    was painted; the distance look of the same call is complete."""

    def __init__(self, message, work, limit):
        super().__init__(message)
        self.work, self.limit = int(work), int(limit)


class SkeletonLimitError(EngineError):
    """A skeleton look that ran out of sub-iterations (CHS_ELIMIT): a pixel was still deleted in sub-iteration ``subiters``,
    within the last four of the ``limit`` the caller allowed.  There is no skeleton result; the distance look of the same
    call is complete."""

    def __init__(self, message, subiters, limit):
        super().__init__(message)
        self.subiters, self.limit = int(subiters), int(limit)


class GeodesicLimitError(EngineError):
    """A geodesic look that ran out of rounds (CHS_ELIMIT): tiles were still active after ``rounds`` relaxation rounds, the
    caller allowed ``limit``.  There is no geodesic result; the components look of the same call is complete."""

    def __init__(self, message, rounds, limit):
        super().__init__(message)
        self.rounds, self.limit = int(rounds), int(limit)


class TransportLimitError(EngineError):
    """A transport look that ran out of iterations (CHS_ELIMIT): the solve was not accepted after ``iters`` conjugate-gradient
    iterations, the caller allowed ``limit``.  There is no transport result; the components look of the same call is
    complete."""

    def __init__(self, message, iters, limit):
        super().__init__(message)
        self.iters, self.limit = int(iters), int(limit)


_lib = None


def resolve_library():
    """The library to load and whether it is the product.  CHS_LIB_PATH selects another build (an experiment
    variant under lib/variants/, tools/ab.sh) -- said aloud on stderr, never silently.  The product library
    (lib/libchs_hip.so) must carry the sha256 of the sources in the tree (chsimpy_amd/_build.py): one that does
    not -- a variant copied over it, a library older than an edit -- is rebuilt when hipcc is at hand and refused
    otherwise (CHS_NO_REBUILD=1: always refused)."""
    import sys
    from . import _build
    override = os.environ.get('CHS_LIB_PATH')
    if override:
        have, flags = _build.embedded_provenance(override)
        sys.stderr.write(f"chsimpy_amd: CHS_LIB_PATH -> {override} (sources {str(have)[:12]}, extra flags '{flags}'): "
                         "NOT the product library\n")
        return override, False
    path = LIB_PATH
    want = _build.source_hash()
    if want is None or not os.path.exists(path):
        return path, True        # no sources to check against (an installed copy) / missing: load() reports it
    have, flags = _build.embedded_provenance(path)
    if have == want and not flags:
        return path, True
    what = (f"{path} was built from other sources than the tree holds (library {str(have)[:12]}, tree {want[:12]}"
            + (f", extra flags '{flags}'" if flags else '') + ")")
    if os.environ.get('CHS_NO_REBUILD') == '1':
        raise EngineError(what + "; rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        _build.build_hip()
    except Exception as e:
        raise EngineError(what + f"; rebuilding it failed: {e}") from e
    return path, True


def load():
    """Load the HIP library once; raise if it (or any declared symbol) is missing or it is not built from the
    sources in the tree."""
    global _lib
    if _lib is not None:
        return _lib
    path, _product = resolve_library()
    if not os.path.exists(path):
        raise EngineError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). chsimpy_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for s in SYMBOLS:
        if not hasattr(lib, s):
            raise EngineError(f"{path} does not export `{s}` (declared in include/chs_hip.h)")
    dp = C.POINTER(C.c_double)
    lib.chs_create.argtypes = [C.POINTER(chs_consts), dp, C.POINTER(C.c_void_p)]
    lib.chs_destroy.argtypes = [C.c_void_p]
    lib.chs_set_U.argtypes = [C.c_void_p, dp]
    lib.chs_get_U.argtypes = [C.c_void_p, dp]
    lib.chs_prepare.argtypes = [C.c_void_p, dp]
    lib.chs_step_n.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, C.POINTER(C.c_int64)]
    lib.chs_get_state.argtypes = [C.c_void_p, C.POINTER(chs_state)]
    lib.chs_set_state.argtypes = [C.c_void_p, C.POINTER(chs_state)]
    lib.chs_set_jitter_noise.argtypes = [C.c_void_p, C.c_double, dp]
    lib.chs_set_jitter_pcg64.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.chs_init_U_pcg64.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.chs_dctn.argtypes = [C.c_void_p, dp, dp, C.c_int]
    lib.chs_get_mu.argtypes = [C.c_void_p, dp]
    lib.chs_engine.argtypes = [C.c_void_p]
    lib.chs_test_math.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_int64]
    lib.chs_test_math_cols.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_int64]
    lib.chs_kernel_name.argtypes = [C.c_void_p, C.c_int]
    lib.chs_kernel_name.restype = C.c_char_p
    lib.chs_profile_steps.argtypes = [C.c_void_p, C.c_int64, dp, C.POINTER(C.c_int64)]
    lib.chs_last_step_ms.argtypes = [C.c_void_p]
    lib.chs_last_step_ms.restype = C.c_double
    lib.chs_last_error.restype = C.c_char_p
    lib.chs_version.restype = C.c_char_p
    lib.chs_pool_clear.argtypes = []
    vp, u64p, i64p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    lib.chs_batch_create.argtypes = [C.POINTER(chs_consts), C.c_int32, dp, C.POINTER(C.c_void_p)]
    lib.chs_batch_destroy.argtypes = [vp]
    lib.chs_batch_engine.argtypes = [vp]
    lib.chs_batch_set_U.argtypes = [vp, C.c_int32, dp]
    lib.chs_batch_init_U_pcg64.argtypes = [vp, C.c_int32, C.c_double, C.c_double, u64p, u64p]
    lib.chs_batch_get_U.argtypes = [vp, C.c_int32, dp]
    lib.chs_batch_prepare.argtypes = [vp, dp]
    lib.chs_batch_step_n.argtypes = [vp, i64p, C.c_int32, dp, i64p, C.POINTER(C.c_int32)]
    lib.chs_batch_get_state.argtypes = [vp, C.c_int32, C.POINTER(chs_state)]
    lib.chs_batch_set_state.argtypes = [vp, C.c_int32, C.POINTER(chs_state)]
    lib.chs_batch_step_n_queued.argtypes = [vp, C.c_int32, i64p, C.c_int32, i64p, C.POINTER(C.c_int32)]
    lib.chs_batch_member_rows.argtypes = [vp, C.c_int32, dp, C.c_int64]
    lib.chs_structure_factor_bins.argtypes = [C.c_int32]
    lib.chs_structure_factor_bins.restype = C.c_int32
    lib.chs_structure_factor.argtypes = [vp, dp, C.c_int32]
    lib.chs_structure_factor_last_ms.argtypes = [vp, dp]
    lib.chs_batch_structure_factor.argtypes = [vp, C.c_int32, dp, C.c_int32]
    lib.chs_morphology.argtypes = [vp, C.c_double, i64p]
    lib.chs_morphology_last_ms.argtypes = [vp, dp]
    lib.chs_batch_morphology.argtypes = [vp, C.c_int32, dp, i64p]
    i32p = C.POINTER(C.c_int32)
    lib.chs_components.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, i64p]
    lib.chs_components_table.argtypes = [vp, C.c_int64, i32p]
    lib.chs_components_labels.argtypes = [vp, i32p]
    lib.chs_components_last_ms.argtypes = [vp, dp]
    lib.chs_components_tile.argtypes = [i32p, i32p]
    lib.chs_batch_components.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, i64p]
    lib.chs_batch_components_table.argtypes = [vp, C.c_int64, i32p]
    lib.chs_batch_components_labels.argtypes = [vp, i32p]
    lib.chs_distance_bins.argtypes = [C.c_int32]
    lib.chs_distance_bins.restype = C.c_int32
    lib.chs_distance.argtypes = [vp, C.c_double, C.c_int32, i64p]
    lib.chs_distance_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_distance_map.argtypes = [vp, i32p]
    lib.chs_distance_last_ms.argtypes = [vp, dp]
    lib.chs_distance_tile.argtypes = [i32p, i32p]
    lib.chs_batch_distance.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, i64p]
    lib.chs_batch_distance_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_batch_distance_map.argtypes = [vp, i32p]
    lib.chs_chords_bins.argtypes = [C.c_int32]
    lib.chs_chords_bins.restype = C.c_int32
    lib.chs_chords.argtypes = [vp, C.c_double, i64p]
    lib.chs_chords_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_chords_last_ms.argtypes = [vp, dp]
    lib.chs_chords_tile.argtypes = [i32p, i32p, i32p]
    lib.chs_batch_chords.argtypes = [vp, C.c_int32, C.c_double, i64p]
    lib.chs_batch_chords_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_composition.argtypes = [vp, C.c_double, C.c_int32, C.c_double, C.c_double, i64p, dp]
    lib.chs_composition_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_composition_select.argtypes = [vp, C.c_int32, i64p, dp]
    lib.chs_composition_last_ms.argtypes = [vp, dp]
    lib.chs_composition_tile.argtypes = [i32p, i32p, i32p, i32p]
    lib.chs_batch_composition.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_double, i64p, dp]
    lib.chs_batch_composition_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_batch_composition_select.argtypes = [vp, C.c_int32, C.c_int32, i64p, dp]
    lib.chs_batch_composition_last_ms.argtypes = [vp, dp]
    lib.chs_two_point_max_r.argtypes = [C.c_int32]
    lib.chs_two_point_max_r.restype = C.c_int32
    lib.chs_two_point_size.argtypes = [C.c_int32, C.c_int32]
    lib.chs_two_point_size.restype = C.c_int64
    lib.chs_two_point.argtypes = [vp, C.c_double, C.c_int32, i64p]
    lib.chs_two_point_counts.argtypes = [vp, C.c_int64, i64p]
    lib.chs_two_point_last_ms.argtypes = [vp, dp]
    lib.chs_two_point_tile.argtypes = [i32p, i32p, i32p]
    lib.chs_batch_two_point.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, i64p]
    lib.chs_batch_two_point_counts.argtypes = [vp, C.c_int64, i64p]
    lib.chs_batch_two_point_last_ms.argtypes = [vp, dp]
    lib.chs_contour.argtypes = [vp, C.c_double, C.c_int32, C.c_double, C.c_int32, i64p, dp]
    lib.chs_contour_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_contour_map.argtypes = [vp, C.c_int64, dp]
    lib.chs_contour_last_ms.argtypes = [vp, dp]
    lib.chs_contour_tile.argtypes = [i32p, i32p, i32p, i32p]
    lib.chs_batch_contour.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_int32, i64p, dp]
    lib.chs_batch_contour_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_batch_contour_map.argtypes = [vp, C.c_int64, dp]
    lib.chs_batch_contour_last_ms.argtypes = [vp, dp]
    lib.chs_shapes.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, i64p]
    lib.chs_shapes_table.argtypes = [vp, C.c_int64, i64p]
    lib.chs_shapes_last_ms.argtypes = [vp, dp]
    lib.chs_batch_shapes.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, i64p]
    lib.chs_batch_shapes_table.argtypes = [vp, C.c_int64, i64p]
    lib.chs_track.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, C.c_int32, i64p]
    lib.chs_track_pairs.argtypes = [vp, C.c_int64, i64p]
    lib.chs_track_reset.argtypes = [vp]
    lib.chs_track_last_ms.argtypes = [vp, dp]
    lib.chs_thickness_work_default.argtypes = [C.c_int32]
    lib.chs_thickness_work_default.restype = C.c_int64
    lib.chs_thickness_reach.argtypes = [C.c_int32, C.c_int32]
    lib.chs_thickness_reach.restype = C.c_int32
    lib.chs_thickness.argtypes = [vp, C.c_double, C.c_int32, C.c_int64, i64p]
    lib.chs_thickness_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_thickness_map.argtypes = [vp, i32p]
    lib.chs_thickness_last_ms.argtypes = [vp, dp]
    lib.chs_batch_thickness.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int64, i64p]
    lib.chs_batch_thickness_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_batch_thickness_map.argtypes = [vp, i32p]
    lib.chs_batch_thickness_last_ms.argtypes = [vp, dp]
    lib.chs_geodesic_bins.argtypes = [C.c_int32]
    lib.chs_geodesic_bins.restype = C.c_int32
    lib.chs_geodesic_rounds_default.argtypes = [C.c_int32]
    lib.chs_geodesic_rounds_default.restype = C.c_int64
    lib.chs_geodesic.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int64, i64p]
    lib.chs_geodesic_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_geodesic_profile.argtypes = [vp, i64p]
    lib.chs_geodesic_map.argtypes = [vp, i32p]
    lib.chs_geodesic_last_ms.argtypes = [vp, dp]
    lib.chs_geodesic_relax_ms.argtypes = [vp, dp]
    lib.chs_batch_geodesic.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int64, i64p]
    lib.chs_batch_geodesic_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_batch_geodesic_profile.argtypes = [vp, i64p]
    lib.chs_batch_geodesic_map.argtypes = [vp, i32p]
    lib.chs_batch_geodesic_last_ms.argtypes = [vp, dp]
    lib.chs_transport_iters_default.argtypes = [C.c_int32]
    lib.chs_transport_iters_default.restype = C.c_int64
    lib.chs_transport.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_int64, i64p, dp]
    lib.chs_transport_profile.argtypes = [vp, dp]
    lib.chs_transport_map.argtypes = [vp, dp]
    lib.chs_transport_last_ms.argtypes = [vp, dp]
    lib.chs_transport_solve_ms.argtypes = [vp, dp]
    lib.chs_batch_transport.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_int64, i64p, dp]
    lib.chs_batch_transport_profile.argtypes = [vp, dp]
    lib.chs_batch_transport_map.argtypes = [vp, dp]
    lib.chs_batch_transport_last_ms.argtypes = [vp, dp]
    lib.chs_batch_transport_solve_ms.argtypes = [vp, dp]
    lib.chs_skeleton_subiters_default.argtypes = [C.c_int32]
    lib.chs_skeleton_subiters_default.restype = C.c_int64
    lib.chs_skeleton.argtypes = [vp, C.c_double, C.c_int32, C.c_int64, i64p]
    lib.chs_skeleton_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_skeleton_plane.argtypes = [vp, u64p]
    lib.chs_skeleton_last_ms.argtypes = [vp, dp]
    lib.chs_skeleton_thin_ms.argtypes = [vp, dp]
    lib.chs_batch_skeleton.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int64, i64p]
    lib.chs_batch_skeleton_hist.argtypes = [vp, C.c_int32, i64p]
    lib.chs_batch_skeleton_plane.argtypes = [vp, u64p]
    lib.chs_batch_skeleton_last_ms.argtypes = [vp, dp]
    lib.chs_batch_skeleton_thin_ms.argtypes = [vp, dp]
    lib.chs_batch_track.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, i64p]
    lib.chs_batch_track_pairs.argtypes = [vp, C.c_int64, i64p]
    lib.chs_batch_track_reset.argtypes = [vp, C.c_int32]
    # engines parked by chs_destroy are device memory of this process: hand them back at interpreter exit
    import atexit
    atexit.register(lib.chs_pool_clear)
    _lib = lib
    return lib


def pool_clear():
    """Free the engines `chs_destroy` has parked for reuse (include/chs_hip.h: chs_pool_clear)."""
    load().chs_pool_clear()


def pool_count():
    """Number of engines parked for reuse right now."""
    return int(load().chs_pool_count())


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i64ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _i32ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def components_tile():
    """(rows, columns) of the tile a workgroup of chs_components labels in LDS (chs_components_tile)."""
    r, c = C.c_int32(0), C.c_int32(0)
    rc = load().chs_components_tile(C.byref(r), C.byref(c))
    if rc != CHS_OK:
        raise EngineError(f"chs_components_tile failed ({rc})")
    return int(r.value), int(c.value)


def distance_tile():
    """(band_rows, row_chunk) of the kernels of chs_distance (chs_distance_tile): the rows of a band of the vertical pass
    and the consecutive pixels one wavefront pass of the horizontal pass covers."""
    b, c = C.c_int32(0), C.c_int32(0)
    rc = load().chs_distance_tile(C.byref(b), C.byref(c))
    if rc != CHS_OK:
        raise EngineError(f"chs_distance_tile failed ({rc})")
    return int(b.value), int(c.value)


def thickness_work_default(N):
    """The default work limit of chs_thickness at grid size N (chs_thickness_work_default): K N^2."""
    return int(load().chs_thickness_work_default(int(N)))


def thickness_reach(R, diagonal):
    """E(R, axis) or E(R, diagonal) of the pruning rule of chs_thickness, by the function the kernel compiles."""
    return int(load().chs_thickness_reach(int(R), 1 if diagonal else 0))


def geodesic_bins(N):
    """The length of the histogram of chs_geodesic at grid size N (chs_geodesic_bins): 4N."""
    return int(load().chs_geodesic_bins(int(N)))


def skeleton_subiters_default(N):
    """The default limit of the sub-iterations of chs_skeleton at grid size N (chs_skeleton_subiters_default): 4 N + 64."""
    return int(load().chs_skeleton_subiters_default(int(N)))


def transport_iters_default(N):
    """The default iteration limit of chs_transport at grid size N (chs_transport_iters_default): 48 N + 64."""
    return int(load().chs_transport_iters_default(int(N)))


def geodesic_rounds_default(N):
    """The default round limit of chs_geodesic at grid size N (chs_geodesic_rounds_default): 32 nt^2 + 64."""
    return int(load().chs_geodesic_rounds_default(int(N)))


def distance_bins(N):
    """The length of the histogram of chs_distance at grid size N (chs_distance_bins)."""
    return int(load().chs_distance_bins(int(N)))


def chords_tile():
    """(word_bits, lines_per_group, local_bins) of the kernels of chs_chords (chs_chords_tile): the pixels of a line in one
    word, the lines of a workgroup of the walk, and the lengths below which a chord goes to the workgroup's histogram."""
    w, g, b = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = load().chs_chords_tile(C.byref(w), C.byref(g), C.byref(b))
    if rc != CHS_OK:
        raise EngineError(f"chs_chords_tile failed ({rc})")
    return int(w.value), int(g.value), int(b.value)


def chords_bins(N):
    """The bins of each of the eight histograms of chs_chords at grid size N (chs_chords_bins)."""
    return int(load().chs_chords_bins(int(N)))


def two_point_tile():
    """(word_bits, band_rows, lanes) of the kernels of chs_two_point (chs_two_point_tile): the pixels of a row in one word,
    the rows of a band of the pair kernel and the lanes of its workgroup, which owns band_rows rows of CHS_TP_CHUNK pixels."""
    w, h, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = load().chs_two_point_tile(C.byref(w), C.byref(h), C.byref(n))
    if rc != CHS_OK:
        raise EngineError(f"chs_two_point_tile failed ({rc})")
    return int(w.value), int(h.value), int(n.value)


def two_point_max_r(N):
    """The largest rmax of chs_two_point at grid size N (chs_two_point_max_r)."""
    return int(load().chs_two_point_max_r(int(N)))


def two_point_size(N, rmax):
    """The entries of the count table of chs_two_point, 0 for arguments out of range (chs_two_point_size)."""
    return int(load().chs_two_point_size(int(N), int(rmax)))


def composition_tile():
    """(elems_per_thread, threads, max_groups, digit_bits) of the kernels of chs_composition (chs_composition_tile): a
    workgroup of `threads` threads takes tiles of threads * elems_per_thread elements, every max_groups-th one where the
    field has more tiles; the digits of the radix select have digit_bits bits."""
    v = [C.c_int32(0) for _ in range(4)]
    rc = load().chs_composition_tile(*(C.byref(x) for x in v))
    if rc != CHS_OK:
        raise EngineError(f"chs_composition_tile failed ({rc})")
    return tuple(int(x.value) for x in v)


def composition_sum_terms(N, tile=None):
    """(E, D) of the error bound of the float sums of chs_composition at grid size N: the elements
    a thread adds one after the other, and the depth of the trees above it."""
    ept, threads, max_groups, _ = tile or composition_tile()
    tiles = -(-(N * N) // (threads * ept))
    groups = min(tiles, max_groups)
    return ept * -(-tiles // groups), (threads - 1).bit_length() + (max_groups - 1).bit_length()


def contour_tile():
    """(tile_w, tile_h, threads, fin_threads) of the kernels of chs_contour (chs_contour_tile): a workgroup of `threads`
    threads owns tile_w x tile_h cells, and the finishing workgroup has fin_threads threads."""
    v = [C.c_int32(0) for _ in range(4)]
    rc = load().chs_contour_tile(*(C.byref(x) for x in v))
    if rc != CHS_OK:
        raise EngineError(f"chs_contour_tile failed ({rc})")
    return tuple(int(x.value) for x in v)


def contour_sum_terms(N, tile=None):
    """(E, D) of the error bound of the float sums of chs_contour at grid size N: the terms that are
    added one after the other -- a thread's at most two segments of each of its queue entries, then the slots of a thread
    of the finishing workgroup, the first of which is the end of the first chain -- and the depth of the two trees."""
    tw, th, threads, fin = tile or contour_tile()
    tiles = -(-(N - 1) // tw) * -(-(N - 1) // th)
    return 2 * (tw * th // threads) + -(-tiles // fin) - 1, (threads - 1).bit_length() + (fin - 1).bit_length()


def __getattr__(name):
    if name == 'CC_TILE':   # read from the library at the first use: importing the binding does not load it
        return components_tile()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def test_math(which, a, b=None, device=0):
    """Device math primitives (accuracy tests): see chs_test_math in include/chs_hip.h."""
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    out = np.empty_like(a)
    if b is None:
        b = np.zeros(4)
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    rc = lib.chs_test_math(device, which, _dptr(a), _dptr(b), _dptr(out), a.size)
    if rc != CHS_OK:
        raise EngineError(f"chs_test_math failed ({rc}): {lib.chs_last_error().decode()}")
    return out


# codes of chs_test_math_cols (include/chs_hip.h)
MATH_DIV_POS, MATH_DIV_POS1 = 10, 11
MATH_EMU_BOTH, MATH_EMU_ENERGY, MATH_EMU_MU = 12, 13, 14
MATH_CHAIN, MATH_CHAIN_DOM = 15, 16
MATH_E_LOGS, MATH_MU_LOGS, MATH_E_LOGS_FAST, MATH_MU_LOGS_FAST = 17, 18, 19, 20
MATH_E_LOGS_F32, MATH_MU_LOGS_F32, MATH_E_LOGS_FAST_F32, MATH_MU_LOGS_FAST_F32 = 21, 22, 23, 24
MATH_DT, MATH_DT_FAST, MATH_DT_FAST_F32 = 25, 26, 27
MATH_SPECTRAL, MATH_SPECTRAL_F32IO, MATH_SPECTRAL_F32 = 28, 29, 30
MATH_LOGF, MATH_LOG_RATIO_F32, MATH_MU_F32, MATH_ENERGY_F32 = 31, 32, 33, 34
MATH_LOG_TAB_F32, MATH_LOG_TAB = 35, 36
MATH_F32_CODES = (21, 22, 23, 24, 27, 31, 32, 33, 34, 35)   # every input and constant is a float value
MATH_F32_IO_CODES = (29, 30)                                # in0, in1 are float values; li, lj, lam1, lam2 stay double


def test_math_cols(which, cols, consts=(), device=0):
    """One inline function of chs_math.h elementwise on the device: chs_test_math_cols in include/chs_hip.h.  `cols`:
    up to four equally long input columns, `consts`: up to eight uniform constants; returns the two output columns.
    The fp32 codes get every input rounded to float here, so that the device's conversion is exact."""
    lib = load()
    cols = [np.ascontiguousarray(c, dtype=np.float64).ravel() for c in cols]
    if not 1 <= len(cols) <= 4 or any(c.size != cols[0].size for c in cols) or len(consts) > 8:
        raise ValueError("one to four input columns of one length and at most eight constants")
    n = cols[0].size
    k = np.zeros(8)
    k[:len(consts)] = consts
    nf32 = 4 if which in MATH_F32_CODES else 2 if which in MATH_F32_IO_CODES else 0
    if which in MATH_F32_CODES:
        k = k.astype(np.float32).astype(np.float64)
    buf = np.zeros((4, max(n, 1)))
    for j, c in enumerate(cols):
        buf[j, :n] = c.astype(np.float32).astype(np.float64) if j < nf32 else c
    out = np.empty((2, max(n, 1)))
    rc = lib.chs_test_math_cols(device, which, _dptr(buf), _dptr(k), _dptr(out), n)
    if rc != CHS_OK:
        raise EngineError(f"chs_test_math_cols failed ({rc}): {lib.chs_last_error().decode()}")
    return out[0], out[1]


class _Looks:
    """The looks at a thresholded field that go member by member, written once for `Engine` and `Batch`: the same calls
    but for the prefix of the symbol (`_prefix`: ``chs_`` or ``chs_batch_``) and what stands in front of the threshold
    (`lead`: nothing, or the member).  A batch has one set of buffers, so what is fetched is that of its last look."""

    _cmp_nbins = 0

    def _look_call(self, name, *args):
        what = self._prefix + name
        self._check(getattr(self.lib, what)(self._h, *args), what)

    def _last_ms(self, symbol):
        """Device time (ms) of the last look of a kind, by the symbol that answers it."""
        ms = C.c_double(0.0)
        self._check(getattr(self.lib, symbol)(self._h, C.byref(ms)), symbol)
        return float(ms.value)

    def _components(self, lead, threshold, connectivity, side):
        out = np.empty(CHS_CC_WORDS, dtype=np.int64)
        self._look_call('components', *lead, float(threshold), int(connectivity), int(side), _i64ptr(out))
        self._cc_count = int(out[0])
        return out

    def components_table(self):
        """int32 [count][6] of the last look: first, area, imin, imax, jmin, jmax."""
        out = np.empty((self._cc_count, CHS_CC_COLS), dtype=np.int32)
        self._look_call('components_table', self._cc_count, _i32ptr(out))
        return out

    def components_labels(self):
        """int32 [N][N] of the last look: the component's number, -1 for background."""
        out = np.empty((self.N, self.N), dtype=np.int32)
        self._look_call('components_labels', _i32ptr(out))
        return out

    def _components_look(self, lead, threshold, connectivity, side, table, labels):
        words = self._components(lead, threshold, connectivity, side)
        return words, (self.components_table() if table else None), (self.components_labels() if labels else None)

    def _distance(self, lead, threshold, side):
        out = np.empty(CHS_DT_WORDS, dtype=np.int64)
        self._look_call('distance', *lead, float(threshold), int(side), _i64ptr(out))
        return out

    def distance_hist(self):
        """int64 [chs_distance_bins(N)] of the last look: the foreground pixels by radius bin."""
        out = np.empty(int(self.lib.chs_distance_bins(self.N)), dtype=np.int64)
        self._look_call('distance_hist', len(out), _i64ptr(out))
        return out

    def distance_map(self):
        """int32 [N][N] of the last look: the squared distances."""
        out = np.empty((self.N, self.N), dtype=np.int32)
        self._look_call('distance_map', _i32ptr(out))
        return out

    def _distance_look(self, lead, threshold, side, hist, map):
        words = self._distance(lead, threshold, side)
        return words, (self.distance_hist() if hist else None), (self.distance_map() if map else None)

    def _thickness(self, lead, threshold, side, max_work):
        out = np.empty(CHS_TH_WORDS, dtype=np.int64)
        limit = 0 if max_work is None else int(max_work)
        what = self._prefix + 'thickness'
        rc = getattr(self.lib, what)(self._h, *lead, float(threshold), int(side), limit, _i64ptr(out))
        if rc == CHS_ELIMIT:
            msg = self.lib.chs_last_error().decode(errors='replace')
            raise ThicknessLimitError(f"{what} refused ({rc}): {msg}", out[CHS_TH_WORK],
                                      limit or self.lib.chs_thickness_work_default(self.N))
        self._check(rc, what)
        return out

    def thickness_hist(self):
        """int64 [chs_distance_bins(N)] of the last thickness look: the foreground pixels by bin of the local radius."""
        out = np.empty(int(self.lib.chs_distance_bins(self.N)), dtype=np.int64)
        self._look_call('thickness_hist', len(out), _i64ptr(out))
        return out

    def thickness_map(self):
        """int32 [N][N] of the last thickness look: the squared local radii."""
        out = np.empty((self.N, self.N), dtype=np.int32)
        self._look_call('thickness_map', _i32ptr(out))
        return out

    def _thickness_look(self, lead, threshold, side, hist, map, max_work):
        """(words, hist, t2) of the thickness look and (words, hist, d2) of its distance look.  The C entry returns the
        thickness words alone, so the five distance words come from a distance look of their own on the same buffers and
        field -- the same bits as the one inside, at a fraction of the thickness look's cost."""
        words = self._thickness(lead, threshold, side, max_work)
        th = words, (self.thickness_hist() if hist else None), (self.thickness_map() if map else None)
        return th, self._distance_look(lead, threshold, side, hist, map)

    def thickness_ms(self):
        """Device time (ms) of the last thickness look, the distance look inside included."""
        return self._last_ms(self._prefix + 'thickness_last_ms')

    def _geodesic(self, lead, threshold, connectivity, side, source, max_rounds):
        out = np.empty(CHS_GEO_WORDS, dtype=np.int64)
        limit = 0 if max_rounds is None else int(max_rounds)
        what = self._prefix + 'geodesic'
        rc = getattr(self.lib, what)(self._h, *lead, float(threshold), int(connectivity), int(side), int(source), limit,
                                     _i64ptr(out))
        if rc == CHS_ELIMIT:
            msg = self.lib.chs_last_error().decode(errors='replace')
            raise GeodesicLimitError(f"{what} refused ({rc}): {msg}", out[CHS_GEO_ROUNDS], out[CHS_GEO_LIMIT])
        self._check(rc, what)
        self._cc_count = int(out[12])                      # CHS_GEO_CC_COUNT (a geodesic look is a components look too)
        return out

    def geodesic_hist(self):
        """int64 [chs_geodesic_bins(N)] of the last geodesic look: the reached pixels by G / UNIT."""
        out = np.empty(int(self.lib.chs_geodesic_bins(self.N)), dtype=np.int64)
        self._look_call('geodesic_hist', len(out), _i64ptr(out))
        return out

    def geodesic_profile(self):
        """int64 [N][3] of the last geodesic look: foreground, reached and the sum of G by depth."""
        out = np.empty((self.N, 3), dtype=np.int64)
        self._look_call('geodesic_profile', _i64ptr(out))
        return out

    def geodesic_map(self):
        """int32 [N][N] of the last geodesic look: G."""
        out = np.empty((self.N, self.N), dtype=np.int32)
        self._look_call('geodesic_map', _i32ptr(out))
        return out

    def _geodesic_look(self, lead, threshold, connectivity, side, source, hist, profile, map, max_rounds):
        """(words, hist or None, profile or None, G or None) of one geodesic look."""
        words = self._geodesic(lead, threshold, connectivity, side, source, max_rounds)
        return (words, self.geodesic_hist() if hist else None, self.geodesic_profile() if profile else None,
                self.geodesic_map() if map else None)

    def geodesic_ms(self):
        """Device time (ms) of the last geodesic look, the components look inside included."""
        return self._last_ms(self._prefix + 'geodesic_last_ms')

    def geodesic_rounds_default(self):
        """The default round limit of a geodesic look at this grid size."""
        return int(self.lib.chs_geodesic_rounds_default(self.N))

    def _skeleton(self, lead, threshold, side, max_subiters):
        out = np.empty(CHS_SK_WORDS, dtype=np.int64)
        limit = 0 if max_subiters is None else int(max_subiters)
        what = self._prefix + 'skeleton'
        rc = getattr(self.lib, what)(self._h, *lead, float(threshold), int(side), limit, _i64ptr(out))
        if rc == CHS_ELIMIT:
            msg = self.lib.chs_last_error().decode(errors='replace')
            raise SkeletonLimitError(f"{what} refused ({rc}): {msg}", out[CHS_SK_SUBITERS], out[CHS_SK_LIMIT])
        self._check(rc, what)
        return out

    def skeleton_hist(self):
        """int64 [chs_distance_bins(N)] of the last skeleton look: the skeleton pixels by bin of their half-width."""
        out = np.empty(int(self.lib.chs_distance_bins(self.N)), dtype=np.int64)
        self._look_call('skeleton_hist', len(out), _i64ptr(out))
        return out

    def skeleton_plane(self):
        """uint64 [N][ceil(N / 64)] of the last skeleton look: the packed skeleton, bit j of word w column 64 w + j."""
        out = np.empty((self.N, (self.N + 63) // 64), dtype=np.uint64)
        self._look_call('skeleton_plane', out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out

    def _skeleton_look(self, lead, threshold, side, hist, map, max_subiters):
        """(words, hist or None, packed plane or None) of one skeleton look."""
        words = self._skeleton(lead, threshold, side, max_subiters)
        return words, (self.skeleton_hist() if hist else None), (self.skeleton_plane() if map else None)

    def skeleton_ms(self):
        """Device time (ms) of the last skeleton look, the distance look inside included."""
        return self._last_ms(self._prefix + 'skeleton_last_ms')

    def skeleton_thin_ms(self):
        """Device time (ms) of the sub-iterations of the last skeleton look."""
        return self._last_ms(self._prefix + 'skeleton_thin_ms')

    def _transport(self, lead, threshold, side, source, tol, max_iters):
        words = np.empty(CHS_TRN_WORDS, dtype=np.int64)
        vals = np.empty(CHS_TRN_VALS, dtype=np.float64)
        limit = 0 if max_iters is None else int(max_iters)
        what = self._prefix + 'transport'
        rc = getattr(self.lib, what)(self._h, *lead, float(threshold), int(side), int(source), float(tol), limit, _i64ptr(words),
                                     _dptr(vals))
        if rc == CHS_ELIMIT:
            msg = self.lib.chs_last_error().decode(errors='replace')
            raise TransportLimitError(f"{what} refused ({rc}): {msg}", words[CHS_TRN_ITERS], words[CHS_TRN_LIMIT])
        self._check(rc, what)
        self._cc_count = int(words[CHS_TRN_CC_COUNT])      # (a transport look is a components look too)
        return words, vals

    def transport_profile(self):
        """float64 [N + 1][3] of the last transport look: cut[k], the sum of c and the active pixels at depth k."""
        out = np.empty((self.N + 1, 3), dtype=np.float64)
        self._look_call('transport_profile', _dptr(out))
        return out

    def transport_map(self):
        """float64 [N][N] of the last transport look: c, -1 on the background, -2 on foreground that is not active."""
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._look_call('transport_map', _dptr(out))
        return out

    def _transport_look(self, lead, threshold, side, source, tol, profile, map, max_iters):
        """(words, vals, profile or None, map or None) of one transport look."""
        words, vals = self._transport(lead, threshold, side, source, tol, max_iters)
        return words, vals, self.transport_profile() if profile else None, self.transport_map() if map else None

    def transport_ms(self):
        """Device time (ms) of the last transport look, the components look inside included."""
        return self._last_ms(self._prefix + 'transport_last_ms')

    def transport_solve_ms(self):
        """Device time (ms) of the iterations and closing sweeps of the last transport look."""
        return self._last_ms(self._prefix + 'transport_solve_ms')

    def transport_iters_default(self):
        """The default iteration limit of a transport look at this grid size."""
        return int(self.lib.chs_transport_iters_default(self.N))

    def _chords(self, lead, threshold):
        out = np.empty(CHS_CH_WORDS, dtype=np.int64)
        self._look_call('chords', *lead, float(threshold), _i64ptr(out))
        return out

    def chords_hist(self):
        """int64 [2][2][2][chs_chords_bins(N)] of the last look: the chords by phase, direction, class and length."""
        nb = int(self.lib.chs_chords_bins(self.N))
        out = np.empty((2, 2, 2, nb), dtype=np.int64)
        self._look_call('chords_hist', nb, _i64ptr(out))
        return out

    def _chords_look(self, lead, threshold, hist):
        words = self._chords(lead, threshold)
        return words, (self.chords_hist() if hist else None)

    def _composition(self, lead, threshold, nbins, lo, hi):
        iw, fw = np.empty(CHS_CMP_IWORDS, dtype=np.int64), np.empty(CHS_CMP_FWORDS, dtype=np.float64)
        self._look_call('composition', *lead, float(threshold), int(nbins), float(lo), float(hi), _i64ptr(iw), _dptr(fw))
        self._cmp_nbins = int(nbins)
        return iw, fw

    def composition_hist(self, nbins=None):
        """int64 [nbins] of the last look: the pixels by bin (nbins: that of the last look of this object)."""
        out = np.empty(self._cmp_nbins if nbins is None else int(nbins), dtype=np.int64)
        self._look_call('composition_hist', len(out), _i64ptr(out))
        return out

    def _composition_look(self, lead, threshold, nbins, lo, hi, hist):
        iw, fw = self._composition(lead, threshold, nbins, lo, hi)
        return iw, fw, (self.composition_hist() if hist else None)

    def _composition_select(self, lead, ranks):
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
        out = np.empty(ranks.size, dtype=np.float64)
        self._look_call('composition_select', *lead, int(ranks.size), _i64ptr(ranks), _dptr(out))
        return out

    def composition_ms(self):
        """Device time (ms) of the last `composition` or `composition_select`."""
        return self._last_ms(self._prefix + 'composition_last_ms')

    _tp_rmax = 0

    def _two_point(self, lead, threshold, rmax):
        out = np.empty(CHS_TP_WORDS, dtype=np.int64)
        self._look_call('two_point', *lead, float(threshold), int(rmax), _i64ptr(out))
        self._tp_rmax = int(rmax)
        return out

    def two_point_counts(self, rmax=None):
        """int64 [2][rmax + 1][2 rmax + 1] of the last look: the pair counts by phase and displacement (rmax: that of the
        last look of this object)."""
        r = self._tp_rmax if rmax is None else int(rmax)
        out = np.empty((2, r + 1, 2 * r + 1), dtype=np.int64)
        self._look_call('two_point_counts', out.size, _i64ptr(out))
        return out

    def _two_point_look(self, lead, threshold, rmax, counts):
        words = self._two_point(lead, threshold, rmax)
        return words, (self.two_point_counts() if counts else None)

    def two_point_ms(self):
        """Device time (ms) of the last `two_point`."""
        return self._last_ms(self._prefix + 'two_point_last_ms')

    @staticmethod
    def two_point_tile():
        return two_point_tile()

    _ct_bins = 0

    def _contour(self, lead, threshold, bins, kmax, map=False):
        words, sums = np.empty(CHS_CT_WORDS, dtype=np.int64), np.empty(CHS_CT_SUMS, dtype=np.float64)
        self._look_call('contour', *lead, float(threshold), int(bins), float(kmax), 1 if map else 0, _i64ptr(words), _dptr(sums))
        self._ct_bins = int(bins)
        return words, sums

    def contour_hist(self, bins=None):
        """int64 [2][bins] of the last look: the curvature cells per bin, then their fix(ell) per bin (bins: that of the
        last look of this object)."""
        out = np.empty((2, self._ct_bins if bins is None else int(bins)), dtype=np.int64)
        self._look_call('contour_hist', out.shape[1], _i64ptr(out))
        return out

    def contour_map(self):
        """float64 [2][N-1][N-1] of the last look, if it was taken with the map: ell per cell, then kappa per cell."""
        out = np.empty((2, self.N - 1, self.N - 1), dtype=np.float64)
        self._look_call('contour_map', out.size, _dptr(out))
        return out

    def _contour_look(self, lead, threshold, bins, kmax, hist, map):
        words, sums = self._contour(lead, threshold, bins, kmax, map)
        return words, sums, (self.contour_hist() if hist else None), (self.contour_map() if map else None)

    def contour_ms(self):
        """Device time (ms) of the last `contour`."""
        return self._last_ms(self._prefix + 'contour_last_ms')

    @staticmethod
    def contour_tile():
        return contour_tile()

    _sh_count = 0

    def _shapes(self, lead, threshold, connectivity, side):
        out = np.empty(CHS_SH_WORDS, dtype=np.int64)
        self._look_call('shapes', *lead, float(threshold), int(connectivity), int(side), _i64ptr(out))
        self._sh_count = self._cc_count = int(out[0])      # (a shapes look is a components look too)
        return out

    def shapes_table(self):
        """int64 [count][16] of the last shapes look (chsimpy_amd/shapes.py names the columns)."""
        out = np.empty((self._sh_count, CHS_SH_COLS), dtype=np.int64)
        self._look_call('shapes_table', self._sh_count, _i64ptr(out))
        return out

    def _shapes_look(self, lead, threshold, connectivity, side, labels):
        words = self._shapes(lead, threshold, connectivity, side)
        return words, self.shapes_table(), self.components_table(), (self.components_labels() if labels else None)

    _tr_pairs = 0

    def _track(self, lead, threshold, connectivity, side, keep):
        out = np.empty(CHS_TR_WORDS, dtype=np.int64)
        self._look_call('track', *lead, float(threshold), int(connectivity), int(side), 1 if keep else 0, _i64ptr(out))
        self._sh_count = self._cc_count = int(out[0])      # (a track look is a shapes and a components look too)
        self._tr_pairs = int(out[19])                      # CHS_TR_PAIRS
        return out

    def track_pairs(self):
        """int64 [pairs][3] of the last track look: the rows (a, b, n), sorted by (a, b)."""
        out = np.empty((self._tr_pairs, 3), dtype=np.int64)
        self._look_call('track_pairs', self._tr_pairs, _i64ptr(out))
        return out

    def _track_look(self, lead, threshold, connectivity, side, keep):
        words = self._track(lead, threshold, connectivity, side, keep)
        return words, self.track_pairs(), self.shapes_table(), self.components_table()

    def _track_reset(self, lead):
        self._look_call('track_reset', *lead)

    @staticmethod
    def two_point_max_r(N):
        return two_point_max_r(N)


class Engine(_Looks):
    """One device-resident simulation (an opaque ``chs_handle``)."""
    _prefix = 'chs_'

    def __init__(self, consts: chs_consts, lam):
        self.lib = load()
        self.N = int(consts.N)
        self._h = C.c_void_p()
        self._cc_count = 0
        lam = _as_f64(lam, (self.N,))
        rc = self.lib.chs_create(C.byref(consts), _dptr(lam), C.byref(self._h))
        self._check(rc, 'chs_create')

    # -- error mapping --------------------------------------------------------
    def _check(self, rc, what):
        if rc == CHS_OK:
            return
        msg = self.lib.chs_last_error().decode(errors='replace')
        if rc == CHS_ENAN:
            raise AssertionError(f"{what}: {msg}")  # the reference asserts (timedata.py:10)
        if rc == CHS_ESTATE:
            raise AssertionError(f"{what}: {msg}")  # solver.py:139
        raise EngineError(f"{what} failed ({rc}): {msg}")

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.chs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- field ----------------------------------------------------------------
    def set_U(self, U):
        U = _as_f64(U, (self.N, self.N))
        self._check(self.lib.chs_set_U(self._h, _dptr(U)), 'chs_set_U')

    def get_U(self):
        U = np.empty((self.N, self.N), dtype=np.float64)
        self._check(self.lib.chs_get_U(self._h, _dptr(U)), 'chs_get_U')
        return U

    # -- loop -----------------------------------------------------------------
    def prepare(self):
        row = np.empty(9, dtype=np.float64)
        self._check(self.lib.chs_prepare(self._h, _dptr(row)), 'chs_prepare')
        return row

    def step_n(self, nsteps, carry_hat=False, rederive_hat=False, last_call=False, keep_t1=False):
        """Returns (rows[k,9], rc) -- rc is CHS_OK or CHS_ENAN (rows then end with the NaN row)."""
        nsteps = int(max(nsteps, 0))
        rows = np.empty((max(nsteps, 1), 9), dtype=np.float64)
        done = C.c_int64(0)
        rc = self.lib.chs_step_n(self._h, nsteps, (CHS_STEP_CARRY_HAT if carry_hat else 0) | (CHS_STEP_REDERIVE_HAT if rederive_hat else 0)
                                 | (CHS_STEP_LAST_CALL if last_call else 0) | (CHS_STEP_KEEP_T1 if keep_t1 else 0),
                                 _dptr(rows), C.byref(done))
        if rc not in (CHS_OK, CHS_ENAN):
            self._check(rc, 'chs_step_n')
        return rows[:done.value].copy(), rc

    def get_state(self):
        s = chs_state()
        self._check(self.lib.chs_get_state(self._h, C.byref(s)), 'chs_get_state')
        return s

    def set_state(self, s):
        self._check(self.lib.chs_set_state(self._h, C.byref(s)), 'chs_set_state')

    def set_jitter_noise(self, jitter, noise):
        if noise is None:
            self._check(self.lib.chs_set_jitter_noise(self._h, float(jitter or 0.0), None), 'chs_set_jitter_noise')
        else:
            noise = _as_f64(noise, (self.N, self.N))
            self._check(self.lib.chs_set_jitter_noise(self._h, float(jitter), _dptr(noise)), 'chs_set_jitter_noise')

    def init_U_pcg64(self, base, scale, state, inc):
        """U = base + scale*(rand - 0.5) drawn on the device from numpy's PCG64 stream (chs_init_U_pcg64)."""
        m64 = (1 << 64) - 1
        st = (C.c_uint64 * 2)((int(state) >> 64) & m64, int(state) & m64)
        ic = (C.c_uint64 * 2)((int(inc) >> 64) & m64, int(inc) & m64)
        self._check(self.lib.chs_init_U_pcg64(self._h, float(base), float(scale), st, ic), 'chs_init_U_pcg64')

    def set_jitter_pcg64(self, jitter, state, inc):
        """Jitter noise drawn on the device from numpy's PCG64 stream: `state`, `inc` = the two 128-bit
        integers of ``Generator.bit_generator.state['state']``."""
        m64 = (1 << 64) - 1
        st = (C.c_uint64 * 2)((int(state) >> 64) & m64, int(state) & m64)
        ic = (C.c_uint64 * 2)((int(inc) >> 64) & m64, int(inc) & m64)
        self._check(self.lib.chs_set_jitter_pcg64(self._h, float(jitter), st, ic), 'chs_set_jitter_pcg64')

    # -- hooks ----------------------------------------------------------------
    def dctn(self, X, inverse=False):
        X = _as_f64(X, (self.N, self.N))
        Y = np.empty_like(X)
        self._check(self.lib.chs_dctn(self._h, _dptr(X), _dptr(Y), 1 if inverse else 0), 'chs_dctn')
        return Y

    def get_mu(self):
        M = np.empty((self.N, self.N), dtype=np.float64)
        self._check(self.lib.chs_get_mu(self._h, _dptr(M)), 'chs_get_mu')
        return M

    def structure_factor(self):
        """Ssum[nb] of the field the device holds (chs_structure_factor; chsimpy_amd/spectrum.py derives the rest)."""
        nb = int(self.lib.chs_structure_factor_bins(self.N))
        ssum = np.empty(nb, dtype=np.float64)
        self._check(self.lib.chs_structure_factor(self._h, _dptr(ssum), nb), 'chs_structure_factor')
        return ssum

    def structure_factor_ms(self):
        """Device time (ms) of the last `structure_factor`: [sweeps, transform, binning]."""
        ms = np.zeros(3, dtype=np.float64)
        self._check(self.lib.chs_structure_factor_last_ms(self._h, _dptr(ms)), 'chs_structure_factor_last_ms')
        return ms

    def morphology(self, threshold):
        """The seven int64 words Q0, Q1, Q2, QD, Q3, Q4, border of the field the device holds at `threshold`
        (chs_morphology; chsimpy_amd/morphology.py derives the rest)."""
        out = np.empty(CHS_MORPH_WORDS, dtype=np.int64)
        self._check(self.lib.chs_morphology(self._h, float(threshold), _i64ptr(out)), 'chs_morphology')
        return out

    def components(self, threshold, connectivity=4, side=CHS_CC_BELOW):
        """The seven int64 summary words of the connected components of the field the device holds (chs_components;
        chsimpy_amd/components.py names them).  Table and labels of this look: `components_table`, `components_labels`."""
        return self._components((), threshold, connectivity, side)

    def components_look(self, threshold, connectivity, side, table=True, labels=False):
        """One look with what belongs to it: (words, table or None, labels or None)."""
        return self._components_look((), threshold, connectivity, side, table, labels)

    def distance(self, threshold, side=CHS_CC_BELOW):
        """The five int64 summary words of the distance transform of the field the device holds (chs_distance;
        chsimpy_amd/distance.py names them).  Histogram and map of this look: `distance_hist`, `distance_map`."""
        return self._distance((), threshold, side)

    def distance_look(self, threshold, side, hist=True, map=False):
        """One look with what belongs to it: (words, histogram or None, map or None)."""
        return self._distance_look((), threshold, side, hist, map)

    def chords(self, threshold):
        """The 24 int64 summary words of the chord lengths of the field the device holds (chs_chords;
        chsimpy_amd/chords.py names them).  The histograms of this look: `chords_hist`."""
        return self._chords((), threshold)

    def chords_look(self, threshold, hist=True):
        """One look with what belongs to it: (words, histograms or None)."""
        return self._chords_look((), threshold, hist)

    def composition(self, threshold, nbins=15, lo=float('nan'), hi=float('nan')):
        """The int64 and the float64 words of the composition of the field the device holds (chs_composition;
        chsimpy_amd/composition.py names them); lo and hi both NaN: the field's own range.  The histogram of this look:
        `composition_hist`."""
        return self._composition((), threshold, nbins, lo, hi)

    def composition_look(self, threshold, nbins=15, lo=float('nan'), hi=float('nan'), hist=True):
        """One look with what belongs to it: (integer words, float words, histogram or None)."""
        return self._composition_look((), threshold, nbins, lo, hi, hist)

    def composition_select(self, ranks):
        """The ranks[k]-th smallest pixels (0-based, at most CHS_CMP_MAX_RANKS of them), exactly
        (chs_composition_select)."""
        return self._composition_select((), ranks)

    def two_point(self, threshold, rmax):
        """The 8 int64 summary words of the two-point correlation of the field the device holds (chs_two_point;
        chsimpy_amd/two_point.py names them).  The count table of this look: `two_point_counts`."""
        return self._two_point((), threshold, rmax)

    def two_point_look(self, threshold, rmax, counts=True):
        """One look with what belongs to it: (words, count table or None)."""
        return self._two_point_look((), threshold, rmax, counts)

    def contour(self, threshold, bins=64, kmax=1.0, map=False):
        """The 16 int64 words and the 6 float64 sums of the contour of the field the device holds (chs_contour;
        chsimpy_amd/contour.py names them).  The histograms and the map of this look: `contour_hist`, `contour_map`."""
        return self._contour((), threshold, bins, kmax, map)

    def contour_look(self, threshold, bins=64, kmax=1.0, hist=True, map=False):
        """One look with what belongs to it: (words, sums, histograms or None, map or None)."""
        return self._contour_look((), threshold, bins, kmax, hist, map)

    def shapes(self, threshold, connectivity=4, side=CHS_CC_BELOW):
        """The 17 int64 summary words of the droplet shapes of the field the device holds (chs_shapes;
        chsimpy_amd/shapes.py names them).  The table of this look: `shapes_table`; it is a components look as well."""
        return self._shapes((), threshold, connectivity, side)

    def thickness(self, threshold, side=CHS_CC_BELOW, max_work=None):
        """The seven int64 summary words of the local thickness of the field the device holds (chs_thickness;
        chsimpy_amd/thickness.py names them).  Histogram and map of this look: `thickness_hist`, `thickness_map`; it is a
        distance look as well.  A look above `max_work` (None: the default) raises `ThicknessLimitError`."""
        return self._thickness((), threshold, side, max_work)

    def thickness_look(self, threshold, side, hist=True, map=False, max_work=None):
        return self._thickness_look((), threshold, side, hist, map, max_work)

    def geodesic(self, threshold, connectivity=8, side=CHS_CC_BELOW, source=0, max_rounds=None):
        """The sixteen int64 words of the geodesic look at the field the device holds (chs_geodesic;
        chsimpy_amd/geodesic.py names them).  Histogram, profile and map of this look: `geodesic_hist`,
        `geodesic_profile`, `geodesic_map`; it is a components look as well.  A look that needs more than `max_rounds`
        rounds (None: the default) raises `GeodesicLimitError`."""
        return self._geodesic((), threshold, connectivity, side, source, max_rounds)

    def geodesic_look(self, threshold, connectivity, side, source, hist=True, profile=True, map=False, max_rounds=None):
        return self._geodesic_look((), threshold, connectivity, side, source, hist, profile, map, max_rounds)

    def transport(self, threshold, side=CHS_CC_BELOW, source=0, tol=1e-6, max_iters=None):
        """(words, vals) of the transport look at the field the device holds (chs_transport; chsimpy_amd/transport.py
        names them).  Profile and map of this look: `transport_profile`, `transport_map`; it is a components look as
        well.  A solve that is not accepted within `max_iters` iterations (None: the default) raises
        `TransportLimitError`."""
        return self._transport((), threshold, side, source, tol, max_iters)

    def transport_look(self, threshold, side, source, tol=1e-6, profile=True, map=False, max_iters=None):
        return self._transport_look((), threshold, side, source, tol, profile, map, max_iters)

    def geodesic_relax_ms(self):
        """Device time (ms) of the relaxation rounds of the last geodesic look."""
        return self._last_ms('chs_geodesic_relax_ms')

    def skeleton(self, threshold, side=CHS_CC_BELOW, max_subiters=None):
        """The seventeen int64 words of the skeleton look at the field the device holds (chs_skeleton;
        chsimpy_amd/skeleton.py names them).  Histogram and packed plane of this look: `skeleton_hist`, `skeleton_plane`; it
        is a distance look as well.  A look that needs more than `max_subiters` sub-iterations (None: the default) raises
        `SkeletonLimitError`."""
        return self._skeleton((), threshold, side, max_subiters)

    def skeleton_look(self, threshold, side, hist=True, map=False, max_subiters=None):
        return self._skeleton_look((), threshold, side, hist, map, max_subiters)

    def shapes_look(self, threshold, connectivity, side, labels=False):
        """One look with what belongs to it: (words, shape table, component table, labels or None)."""
        return self._shapes_look((), threshold, connectivity, side, labels)

    def shapes_ms(self):
        """Device time (ms) of the sweep and the summary of the last `shapes`."""
        return self._last_ms('chs_shapes_last_ms')

    def track(self, threshold, connectivity=4, side=CHS_CC_BELOW, keep=True):
        """The 25 int64 words of a track look at the field the device holds (chs_track; chsimpy_amd/tracking.py names
        them).  The pair table of this look: `track_pairs`; it is a shapes and a components look as well."""
        return self._track((), threshold, connectivity, side, keep)

    def track_look(self, threshold, connectivity, side, keep=True):
        """(words, pairs, shape table, component table) of one track look."""
        return self._track_look((), threshold, connectivity, side, keep)

    def track_reset(self):
        """Drop the frame (chs_track_reset): the next track look finds none."""
        self._track_reset(())

    def track_ms(self):
        """Device time (ms) of the overlap passes of the last `track`."""
        return self._last_ms('chs_track_last_ms')

    def morphology_ms(self):
        """Device time (ms) of the last `morphology`."""
        return self._last_ms('chs_morphology_last_ms')

    def components_ms(self):
        """Device time (ms) of the last `components`."""
        return self._last_ms('chs_components_last_ms')

    def distance_ms(self):
        """Device time (ms) of the last `distance`."""
        return self._last_ms('chs_distance_last_ms')

    def chords_ms(self):
        """Device time (ms) of the last `chords`."""
        return self._last_ms('chs_chords_last_ms')

    @property
    def engine(self):
        return {CHS_ENGINE_DIRECT: 'direct', CHS_ENGINE_FAST: 'fast', CHS_ENGINE_CHIRP: 'chirp'}[self.lib.chs_engine(self._h)]

    def kernel_names(self):
        out = []
        for i in range(CHS_NKERNELS):
            n = self.lib.chs_kernel_name(self._h, i)
            out.append(n.decode() if n else None)
        return out

    def profile_steps(self, nsteps):
        ms = np.zeros(CHS_NKERNELS, dtype=np.float64)
        calls = np.zeros(CHS_NKERNELS, dtype=np.int64)
        rc = self.lib.chs_profile_steps(self._h, int(nsteps), _dptr(ms), calls.ctypes.data_as(C.POINTER(C.c_int64)))
        self._check(rc, 'chs_profile_steps')
        return ms, calls

    def last_step_ms(self):
        return float(self.lib.chs_last_step_ms(self._h))


def _u128_pair(x):
    m64 = (1 << 64) - 1
    return (C.c_uint64 * 2)((int(x) >> 64) & m64, int(x) & m64)


class Batch(_Looks):
    """B device-resident simulations of one N, dtype and device advanced together (an opaque ``chs_batch``):
    every step kernel is launched once for all members.  Member-wise the methods are those of `Engine`."""
    _prefix = 'chs_batch_'

    def __init__(self, consts_list, lam):
        self.lib = load()
        self.B = len(consts_list)
        self.N = int(consts_list[0].N) if self.B else 0
        self._h = C.c_void_p()
        self._cc_count = 0
        arr = (chs_consts * max(self.B, 1))(*consts_list)
        lam = _as_f64(lam, (self.N,))
        self._check(self.lib.chs_batch_create(arr, self.B, _dptr(lam), C.byref(self._h)), 'chs_batch_create')

    _check = Engine._check

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.chs_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def engine(self):
        """The engine the batch's members run on the device, 'fast' or 'chirp' (chs_batch_engine)."""
        return {CHS_ENGINE_FAST: 'fast', CHS_ENGINE_CHIRP: 'chirp'}[self.lib.chs_batch_engine(self._h)]

    def set_U(self, member, U):
        U = _as_f64(U, (self.N, self.N))
        self._check(self.lib.chs_batch_set_U(self._h, int(member), _dptr(U)), 'chs_batch_set_U')

    def init_U_pcg64(self, member, base, scale, state, inc):
        self._check(self.lib.chs_batch_init_U_pcg64(self._h, int(member), float(base), float(scale), _u128_pair(state),
                                                    _u128_pair(inc)), 'chs_batch_init_U_pcg64')

    def get_U(self, member):
        U = np.empty((self.N, self.N), dtype=np.float64)
        self._check(self.lib.chs_batch_get_U(self._h, int(member), _dptr(U)), 'chs_batch_get_U')
        return U

    def prepare(self):
        """[B, 9] step-0 records; raises like `Engine.prepare` when one of them is NaN."""
        rows = np.empty((self.B, 9), dtype=np.float64)
        self._check(self.lib.chs_batch_prepare(self._h, _dptr(rows)), 'chs_batch_prepare')
        return rows

    def _call(self, what, nsteps, issue):
        """What `step_n` and `step_n_queued` share: the counts with their length check, `done` and `status`, the call
        itself -- `issue(counts, n, done, status)` with the three arrays as the C ABI takes them, returning (rc, anything)
        -- and its rc raised unless it is a member's NaN.  Returns (done, per-member rc, anything)."""
        counts = np.ascontiguousarray([max(int(k), 0) for k in nsteps], dtype=np.int64)
        if counts.size != self.B:
            raise ValueError(f"nsteps needs {self.B} entries, got {counts.size}")
        done = np.zeros(self.B, dtype=np.int64)
        status = np.zeros(self.B, dtype=np.int32)
        rc, extra = issue(counts, counts.ctypes.data_as(C.POINTER(C.c_int64)), done.ctypes.data_as(C.POINTER(C.c_int64)),
                          status.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc not in (CHS_OK, CHS_ENAN):
            self._check(rc, what)
        return done, [int(x) for x in status], extra

    def step_n(self, nsteps):
        """One literal call for every member: nsteps[m] iterations of member m.  Returns (list of rows[k_m, 9],
        list of per-member rc -- CHS_OK or CHS_ENAN, the rows then end with the NaN row)."""
        def issue(counts, n, done, status):
            mx = int(counts.max()) if counts.size else 0
            rows = np.empty((self.B, max(mx, 1), 9), dtype=np.float64)
            return self.lib.chs_batch_step_n(self._h, n, 0, _dptr(rows), done, status), rows
        done, status, rows = self._call('chs_batch_step_n', nsteps, issue)
        return [rows[m, :done[m]].copy() for m in range(self.B)], status

    def step_n_queued(self, nsteps, seats):
        """`step_n` with the members taking turns in `seats` seats on the device (chs_batch_step_n_queued): the same
        return value, bit for bit."""
        def issue(counts, n, done, status):
            return self.lib.chs_batch_step_n_queued(self._h, int(seats), n, 0, done, status), None
        done, status, _ = self._call('chs_batch_step_n_queued', nsteps, issue)
        rows = []
        for m in range(self.B):
            r = np.empty((int(done[m]), 9), dtype=np.float64)
            self._check(self.lib.chs_batch_member_rows(self._h, m, _dptr(r), int(done[m])), 'chs_batch_member_rows')
            rows.append(r)
        return rows, status

    def structure_factor(self, member=None):
        """Ssum of one member ([nb]), or of all of them in one device pass ([B, nb]) for member=None
        (chs_batch_structure_factor with member = -1)."""
        nb = int(self.lib.chs_structure_factor_bins(self.N))
        ssum = np.empty(nb if member is not None else (self.B, nb), dtype=np.float64)
        self._check(self.lib.chs_batch_structure_factor(self._h, -1 if member is None else int(member), _dptr(ssum), nb),
                    'chs_batch_structure_factor')
        return ssum

    def morphology(self, thresholds, member=None):
        """The seven words of one member at the threshold `thresholds` ([7]), or of all members in one device pass at
        their thresholds `thresholds[B]` ([B, 7]) for member=None (chs_batch_morphology with member = -1)."""
        t = _as_f64(np.atleast_1d(thresholds), (1,) if member is not None else (self.B,))
        out = np.empty(CHS_MORPH_WORDS if member is not None else (self.B, CHS_MORPH_WORDS), dtype=np.int64)
        self._check(self.lib.chs_batch_morphology(self._h, -1 if member is None else int(member), _dptr(t), _i64ptr(out)),
                    'chs_batch_morphology')
        return out

    def components(self, member, threshold, connectivity=4, side=CHS_CC_BELOW):
        """`Engine.components` of one member (chs_batch_components)."""
        return self._components((int(member),), threshold, connectivity, side)

    def components_look(self, member, threshold, connectivity, side, table=True, labels=False):
        return self._components_look((int(member),), threshold, connectivity, side, table, labels)

    def distance(self, member, threshold, side=CHS_CC_BELOW):
        """`Engine.distance` of one member (chs_batch_distance)."""
        return self._distance((int(member),), threshold, side)

    def distance_look(self, member, threshold, side, hist=True, map=False):
        return self._distance_look((int(member),), threshold, side, hist, map)

    def chords(self, member, threshold):
        """`Engine.chords` of one member (chs_batch_chords)."""
        return self._chords((int(member),), threshold)

    def chords_look(self, member, threshold, hist=True):
        return self._chords_look((int(member),), threshold, hist)

    def composition(self, member, threshold, nbins=15, lo=float('nan'), hi=float('nan')):
        """`Engine.composition` of one member (chs_batch_composition)."""
        return self._composition((int(member),), threshold, nbins, lo, hi)

    def composition_look(self, member, threshold, nbins=15, lo=float('nan'), hi=float('nan'), hist=True):
        return self._composition_look((int(member),), threshold, nbins, lo, hi, hist)

    def composition_select(self, member, ranks):
        """`Engine.composition_select` of one member (chs_batch_composition_select)."""
        return self._composition_select((int(member),), ranks)

    def two_point(self, member, threshold, rmax):
        """`Engine.two_point` of one member (chs_batch_two_point)."""
        return self._two_point((int(member),), threshold, rmax)

    def two_point_look(self, member, threshold, rmax, counts=True):
        return self._two_point_look((int(member),), threshold, rmax, counts)

    def contour(self, member, threshold, bins=64, kmax=1.0, map=False):
        """`Engine.contour` of one member (chs_batch_contour)."""
        return self._contour((int(member),), threshold, bins, kmax, map)

    def contour_look(self, member, threshold, bins=64, kmax=1.0, hist=True, map=False):
        return self._contour_look((int(member),), threshold, bins, kmax, hist, map)

    def shapes(self, member, threshold, connectivity=4, side=CHS_CC_BELOW):
        """`Engine.shapes` of one member (chs_batch_shapes)."""
        return self._shapes((int(member),), threshold, connectivity, side)

    def thickness(self, member, threshold, side=CHS_CC_BELOW, max_work=None):
        """`Engine.thickness` of one member (chs_batch_thickness)."""
        return self._thickness((int(member),), threshold, side, max_work)

    def thickness_look(self, member, threshold, side, hist=True, map=False, max_work=None):
        return self._thickness_look((int(member),), threshold, side, hist, map, max_work)

    def geodesic(self, member, threshold, connectivity=8, side=CHS_CC_BELOW, source=0, max_rounds=None):
        """`Engine.geodesic` of one member (chs_batch_geodesic)."""
        return self._geodesic((int(member),), threshold, connectivity, side, source, max_rounds)

    def transport(self, member, threshold, side=CHS_CC_BELOW, source=0, tol=1e-6, max_iters=None):
        """`Engine.transport` of one member (chs_batch_transport)."""
        return self._transport((int(member),), threshold, side, source, tol, max_iters)

    def transport_look(self, member, threshold, side, source, tol=1e-6, profile=True, map=False, max_iters=None):
        return self._transport_look((int(member),), threshold, side, source, tol, profile, map, max_iters)

    def geodesic_look(self, member, threshold, connectivity, side, source, hist=True, profile=True, map=False, max_rounds=None):
        return self._geodesic_look((int(member),), threshold, connectivity, side, source, hist, profile, map, max_rounds)

    def skeleton(self, member, threshold, side=CHS_CC_BELOW, max_subiters=None):
        """`Engine.skeleton` of one member (chs_batch_skeleton)."""
        return self._skeleton((int(member),), threshold, side, max_subiters)

    def skeleton_look(self, member, threshold, side, hist=True, map=False, max_subiters=None):
        return self._skeleton_look((int(member),), threshold, side, hist, map, max_subiters)

    def shapes_look(self, member, threshold, connectivity, side, labels=False):
        return self._shapes_look((int(member),), threshold, connectivity, side, labels)

    def track(self, member, threshold, connectivity=4, side=CHS_CC_BELOW, keep=True):
        """`Engine.track` of one member (chs_batch_track): the frame is the member's own."""
        return self._track((int(member),), threshold, connectivity, side, keep)

    def track_look(self, member, threshold, connectivity, side, keep=True):
        return self._track_look((int(member),), threshold, connectivity, side, keep)

    def track_reset(self, member):
        """Drop the frame of one member (chs_batch_track_reset)."""
        self._track_reset((int(member),))

    def get_state(self, member):
        s = chs_state()
        self._check(self.lib.chs_batch_get_state(self._h, int(member), C.byref(s)), 'chs_batch_get_state')
        return s

    def set_state(self, member, s):
        self._check(self.lib.chs_batch_set_state(self._h, int(member), C.byref(s)), 'chs_batch_set_state')
