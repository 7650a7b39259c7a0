"""ctypes binding of libcnf_ot_amd.so -- the C ABI declared in
include/cnf_ot_amd.h.  This is the stub a cnf_ot maintainer would add to call
the MI355X engine from Python.

There is NO CPU fallback: if the HIP library is missing or does not load,
importing the product path fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcnf_ot_amd.so")

CNF_OK = 0
CNF_ERR_INVALID = -22
CNF_ERR_UNSUPPORTED = -95
CNF_ERR_NOMEM = -12
CNF_ERR_HIP = -5


class CnfConfig(ctypes.Structure):
  _fields_ = [
    ("dim", ctypes.c_int32), ("num_layers", ctypes.c_int32),
    ("hidden_size", ctypes.c_int32), ("mlp_num_layers", ctypes.c_int32),
    ("num_bins", ctypes.c_int32),
    ("range_min", ctypes.c_float), ("range_max", ctypes.c_float),
    ("min_bin_size", ctypes.c_float), ("min_knot_slope", ctypes.c_float),
    ("periodized", ctypes.c_int32),
  ]


class CnfFieldGrid(ctypes.Structure):
  _fields_ = [
    ("lo_x", ctypes.c_double), ("lo_y", ctypes.c_double), ("step_x", ctypes.c_double), ("step_y", ctypes.c_double),
    ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("axis_x", ctypes.c_int32), ("axis_y", ctypes.c_int32),
    ("sec_axis", ctypes.c_int32), ("n_sec", ctypes.c_int32),
    ("fixed", ctypes.c_void_p), ("sec", ctypes.c_void_p),
  ]


class CnfLossSpec(ctypes.Structure):
  _fields_ = [
    ("kind", ctypes.c_int32), ("subtype", ctypes.c_int32),
    ("dt", ctypes.c_float), ("dx", ctypes.c_float), ("coef", ctypes.c_float),
    ("a", ctypes.c_float), ("T", ctypes.c_float), ("beta", ctypes.c_float),
  ]


TARGET_MAX_COMP, TARGET_MAX_DIM = 8, 14


class CnfTargetSpec(ctypes.Structure):
  """A Gaussian mixture with a shared covariance shape (include/cnf_ot_amd.h); applications.GaussianMixtureTarget packs it."""
  _fields_ = [
    ("n_comp", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ("mean", (ctypes.c_double * TARGET_MAX_DIM) * TARGET_MAX_COMP),
    ("log_weight", ctypes.c_double * TARGET_MAX_COMP),
    ("W", (ctypes.c_double * TARGET_MAX_DIM) * TARGET_MAX_DIM),
    ("log_det_W", ctypes.c_double),
    ("scale", ctypes.c_void_p),
  ]


MMD_MAX_BW, MMD_MAX_DIM, MMD_MAX_SETS = 8, 14, 64
MMD_KINDS = {"gaussian": 0, "energy": 1}
KNN_MAX_K, KNN_MAX_POINTS = 16, 1 << 20          # CNF_KNN_MAX_K and the largest cloud of cnf_knn


class CnfMmdSpec(ctypes.Structure):
  """The kernel of cnf_mmd2 (include/cnf_ot_amd.h): kind 0 = a sum of Gaussians of n_bw bandwidths, 1 = energy."""
  _fields_ = [("kind", ctypes.c_int32), ("n_bw", ctypes.c_int32), ("bw", ctypes.c_float * MMD_MAX_BW)]


INTERACTION_MAX_TERMS, INTERACTION_MAX_POINTS = 4, 1 << 20
INTERACTION_KINDS = {"gaussian": 0, "exponential": 1, "quadratic": 2, "power": 4}       # (3 is not a kind)
INTERACTION_MAX_EXPONENT = 16.0


class CnfInteractionSpec(ctypes.Structure):
  """The pair kernel of cnf_interaction (include/cnf_ot_amd.h): kind 0 = a signed sum of Gaussians, 1 = of exponentials
  of the distance (Morse), 2 = amp[0] r^2 / 2, 4 = softened power laws and logs with the exponents pw and the softening
  length bw[0]."""
  _fields_ = [("kind", ctypes.c_int32), ("n_terms", ctypes.c_int32), ("amp", ctypes.c_float * INTERACTION_MAX_TERMS),
              ("bw", ctypes.c_float * INTERACTION_MAX_TERMS), ("pw", ctypes.c_float * INTERACTION_MAX_TERMS)]


STEIN_MAX_TERMS = 4
STEIN_KINDS = {"imq": 1, "gaussian": 2}


class CnfSteinSpec(ctypes.Structure):
  """The base kernel of cnf_stein (include/cnf_ot_amd.h): kind 1 = a sum of inverse multiquadrics w_b (bw_b^2 + r^2)^beta,
  2 = a sum of Gaussians w_b exp(-r^2 / (2 bw_b^2))."""
  _fields_ = [("kind", ctypes.c_int32), ("n_terms", ctypes.c_int32), ("w", ctypes.c_float * STEIN_MAX_TERMS),
              ("bw", ctypes.c_float * STEIN_MAX_TERMS), ("beta", ctypes.c_float)]


KDE_MAX_BW = 4


class CnfKdeSpec(ctypes.Structure):
  """The bandwidths of cnf_kde (include/cnf_ot_amd.h) and whether the pair j == i is left out (self mode only)."""
  _fields_ = [("n_bw", ctypes.c_int32), ("loo", ctypes.c_int32), ("bw", ctypes.c_float * KDE_MAX_BW)]


TERM_KINETIC, TERM_KINETIC_SCORE, TERM_FLOW_MATCHING, TERM_POTENTIAL, TERM_REVERSE_KL, TERM_NEG_LOGPROB = range(6)
TERM_DENSITY_L2, TERM_DENSITY_L2_DATA = 6, 7      # evaluation terms (no gradient entry accepts them)
POTENTIALS = {"quadratic": 0, "double_well": 1, "obstacle": 2}
DRIFTS = {"ou": 0, "gradient": 1, "smile": 1, "nongradient": 2, "lorenz": 3}

# name -> (restype, argtypes); every symbol include/cnf_ot_amd.h declares
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_U64 = ctypes.c_uint64
_CFG = ctypes.POINTER(CnfConfig)
SYMBOLS = {
  "cnf_config_default": (None, [_CFG, ctypes.c_int32]),
  "cnf_param_count": (_I64, [_CFG]),
  "cnf_model_create": (ctypes.c_int, [_CFG, ctypes.POINTER(_P)]),
  "cnf_model_destroy": (None, [_P]),
  "cnf_model_set_params": (ctypes.c_int, [_P, _P, _P]),
  "cnf_model_reserve": (ctypes.c_int, [_P, _P, _I64]),
  "cnf_model_reserved": (_I64, [_P, _P]),
  "cnf_model_table_bytes": (_I64, [_P]),
  "cnf_model_has_tables": (ctypes.c_int, [_P]),
  "cnf_model_term_on_tables": (ctypes.c_int, [_P, _I64, _I64, ctypes.c_int]),
  "cnf_model_last_path": (ctypes.c_int, [_P]),
  "cnf_model_set_precise": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_forward_logdet": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P]),
  "cnf_inverse_logdet": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P]),
  "cnf_log_prob": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _P]),
  "cnf_sample_logprob": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P]),
  "cnf_sample_logprob_seeded": (ctypes.c_int, [_P, _U64, _I64, _I64, _P, _I64, _P, _P, _I64, _P]),
  "cnf_forward_logdet_f64": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P]),
  "cnf_inverse_logdet_f64": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P]),
  "cnf_log_prob_f64": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _P]),
  "cnf_sample_logprob_f64": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P]),
  "cnf_fill_normal": (ctypes.c_int, [_U64, _U64, _I64, _P, _P]),
  "cnf_fill_normal_threefry": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, _U64, _U64, _I64, _P, _P, _P]),
  "cnf_loss_terms": (ctypes.c_int, [_P, ctypes.POINTER(CnfLossSpec), _P, ctypes.c_int, _P, _I64, _I64, _P, _P]),
  "cnf_loss_terms_seeded": (ctypes.c_int, [_P, ctypes.POINTER(CnfLossSpec), _U64, _I64, _I64, _P, _I64, _I64, _P, _P]),
  "cnf_grad_supported": (ctypes.c_int, [_CFG]),
  "cnf_grad_enable": (ctypes.c_int, [_P, _I64]),
  "cnf_loss_terms_grad": (ctypes.c_int, [_P, ctypes.POINTER(CnfLossSpec), _P, ctypes.c_int, _P, _I64, _I64,
                                         ctypes.c_float, _P, _P, _P, _P]),
  "cnf_loss_terms_grad_multi": (ctypes.c_int, [_P, ctypes.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
  "cnf_input_vjp": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _I64, _P, _P, _P, _I64, _P]),
  "cnf_pass_vjp": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _I64, _P, _P, _P, _P, _P, _I64, _P]),
  "cnf_neg_logprob_vjp": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.c_float, _P, _P, _P, _I64, _P]),
  "cnf_kinetic_potential_vjp": (ctypes.c_int, [_P, _P, _I64, _P, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_int32,
                                               ctypes.c_float, ctypes.c_float, _P, _P, _P, _P, _P, _P]),
  "cnf_logprob_fd": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.c_float, _P, _I64, _P]),
  "cnf_score": (ctypes.c_int, [_P, _P, ctypes.c_int32, _P, _I64, _I64, _P, _P, _P]),
  "cnf_logprob_fd_vjp": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.c_float, _P, _P, _P, _P, _I64, _P]),
  "cnf_score_fd_vjp": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int32,
                                      ctypes.c_float, ctypes.c_float, _P, _P, _P, _P, _I64, _P]),
  "cnf_score_residual": (ctypes.c_int, [_P, _P, _I64, _I64, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_int32, ctypes.c_float, ctypes.c_float, _P, _P, _P, _P]),
  "cnf_score_residual_force": (ctypes.c_int, [_P, _P, _P, ctypes.c_float, _I64, _I64, ctypes.c_int32, ctypes.c_float,
                                              ctypes.c_float, ctypes.c_int32, ctypes.c_float, ctypes.c_float, _P, _P, _P, _P,
                                              _P]),
  "cnf_term_residual": (ctypes.c_int, [ctypes.c_int32, _P, _P, _I64, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                       ctypes.c_float, _P, _P, _P, _P]),
  "cnf_rkl_residual": (ctypes.c_int, [_P, _P, _I64, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                      ctypes.c_float, _P, _P, _P, _P]),
  "cnf_adam_step": (ctypes.c_int, [_P, _P, _P, _P, _I64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                   ctypes.c_float, _I64, _P]),
  "cnf_step_begin": (ctypes.c_int, [_P, _P]),
  "cnf_fill_normal_dev": (ctypes.c_int, [_P, _U64, _I64, _P, _P]),
  "cnf_fill_uniform_dev": (ctypes.c_int, [_P, _U64, _I64, ctypes.c_float, _P, _P]),
  "cnf_mixture_source_dev": (ctypes.c_int, [_P, _U64, _I64, _P, _P, _P, _P]),
  "cnf_adam_step_dev": (ctypes.c_int, [_P, _P, _P, _P, _I64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_float, _P, _P]),
  "cnf_weighted_sum": (ctypes.c_int, [_P, _P, _I64, _P, _P]),
  "cnf_hopf_cole_workspace": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_double, _I64, _I64,
                                              ctypes.POINTER(_I64)]),
  "cnf_hopf_cole_2d": (ctypes.c_int, [ctypes.c_int32, ctypes.c_float] + [ctypes.c_double] * 6
                       + [_P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
  # the same solution at S times in [0, T] (times: a host array): log_rho [S, n2, n1]; score, drift, vel [S, n2, n1, 2]
  "cnf_hopf_cole_path_workspace": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_double, _I64, _I64,
                                                   ctypes.POINTER(_I64)]),
  "cnf_hopf_cole_path_2d": (ctypes.c_int, [ctypes.c_int32, ctypes.c_float] + [ctypes.c_double] * 6
                            + [ctypes.POINTER(ctypes.c_double), _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P,
                               _I64, _P]),
  "cnf_eulerian_fields": (ctypes.c_int, [_P, ctypes.POINTER(CnfFieldGrid), _P, _I64, _P, _I64, ctypes.c_float, ctypes.c_float,
                                        _P, _P, _P, _P, _P]),
  "cnf_eulerian_fields_f64": (ctypes.c_int, [_P, ctypes.POINTER(CnfFieldGrid), _P, _I64, _P, _I64, ctypes.c_double,
                                            ctypes.c_double, _P, _P, _P, _P, _P]),
  "cnf_trajectories": (ctypes.c_int, [_P, _P, _I64, ctypes.c_float, _P, _I64, ctypes.c_float, _P, _P, _P]),
  "cnf_trajectories_f64": (ctypes.c_int, [_P, _P, _I64, ctypes.c_double, _P, _I64, ctypes.c_double, _P, _P, _P]),
  # the Euler-Maruyama particle reference of the fp problems (snap_step: a host array) and the same statistics of points
  "cnf_fp_particles_workspace": (ctypes.c_int, [_I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_fp_particles": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_double, ctypes.c_double,
                                      _I64, ctypes.c_double, _U64, _I64, _I64, _P, ctypes.POINTER(_I64), ctypes.c_int32,
                                      ctypes.POINTER(CnfFieldGrid), _P, _P, _P, _P, _I64, _P]),
  "cnf_point_stats": (ctypes.c_int, [_P, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(CnfFieldGrid), _P, _P, _P,
                                     _I64, _P]),
  # the finite-volume reference of the 2-D fp problems: coefficient block and rate, K steps per launch, stats [S, 7]
  "cnf_fp_grid_coeffs_bytes": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_fp_grid_coeffs": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_double,
                                        ctypes.POINTER(CnfFieldGrid), _P, _I64, _P, _P]),
  "cnf_fp_grid_steps_workspace": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_fp_grid_steps": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, _I64, ctypes.c_int32, _P, _P,
                                       _I64, _P]),
  "cnf_fp_grid_stats": (ctypes.c_int, [ctypes.POINTER(CnfFieldGrid), _P, ctypes.c_int32, _P, _P]),
  # importance-sampling diagnostics against a closed-form density: stats [n_slices, 5] doubles (m, s1, s2, c, n)
  "cnf_importance_workspace": (ctypes.c_int, [_I64, _I64, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_importance_stats": (ctypes.c_int, [_P, ctypes.POINTER(CnfTargetSpec), _P, ctypes.c_int, _P, _I64, _I64, _P, _P, _I64,
                                          _P]),
  "cnf_importance_stats_seeded": (ctypes.c_int, [_P, ctypes.POINTER(CnfTargetSpec), _U64, _I64, _I64, _P, _I64, _I64, _P, _P,
                                                 _I64, _P]),
  # kernel two-sample statistics of point clouds x [S, N, D], y [S, M, D]: raw sums [S, 3] doubles, xgrad [S, N, D]
  "cnf_mmd_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_mmd_splits": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32]),
  "cnf_mmd2": (ctypes.c_int, [ctypes.POINTER(CnfMmdSpec), ctypes.c_int32, _P, _I64, _P, _I64, ctypes.c_int32, _P, _P, _P,
                              _I64, _P]),
  # the permutation test of the same statistic: labels [N + M, P / 32] words, stats [S, P] doubles, raw [S, P, 2] doubles
  # (q, r) followed by t [S], or NULL
  "cnf_mmd_perm_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_mmd_perm_splits": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32]),
  "cnf_mmd_perm": (ctypes.c_int, [ctypes.POINTER(CnfMmdSpec), ctypes.c_int32, _P, _I64, _P, _I64, ctypes.c_int32, _P,
                                  ctypes.c_int32, _P, _P, _P, _I64, _P]),
  # the Sinkhorn divergence of point clouds (eps: a host array of doubles): sums [S, 6] doubles, potentials
  # [S, 2 N + 2 M], xgrad and xmap [S, N, D]
  "cnf_sinkhorn_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_sinkhorn_splits": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32]),
  "cnf_sinkhorn": (ctypes.c_int, [ctypes.c_int32, _P, _I64, _P, _I64, ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
                                  ctypes.c_int32, _P, _P, _P, _P, _P, _I64, _P]),
  # the sliced Wasserstein distance of point clouds for given directions theta [P, D], G projections at a time: sums
  # [S, P + 2] doubles (the P values, their mean, their maximum), grad [S, N, D]
  "cnf_sliced_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.POINTER(_I64)]),
  "cnf_sliced_tile": (ctypes.c_int, []),
  "cnf_sliced_w2": (ctypes.c_int, [ctypes.c_int32, _P, _I64, _P, _I64, ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int32, _P,
                                   _P, _P, _I64, _P]),
  # the k nearest neighbours of x [S, N, D] in x (self) and in y [S, M, D] (cross): dist, idx [S, N, k] each or NULL,
  # sums [S, 2, k, 2] doubles (block, rank, (sum of log dist over dist > 0, rows with dist == 0))
  "cnf_knn_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_knn_splits": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32]),
  "cnf_knn": (ctypes.c_int, [ctypes.c_int32, _P, _I64, _P, _I64, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P, _P, _P, _I64,
                             _P]),
  # the interaction energy of x [S, N, D] (self mode) or its field at q [S, Q, D]: sums [S] doubles, pot [S, rows] and
  # force [S, rows, D] each or NULL
  "cnf_interaction_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.POINTER(_I64)]),
  "cnf_interaction_splits": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32]),
  "cnf_interaction": (ctypes.c_int, [ctypes.POINTER(CnfInteractionSpec), ctypes.c_int32, _P, _I64, _P, _I64, ctypes.c_int32,
                                     _P, _P, _P, _P, _I64, _P]),
  # the vector-Jacobian product of the self-mode force: x, g, xbar [S, N, D]
  "cnf_interaction_vjp_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_interaction_vjp": (ctypes.c_int, [ctypes.POINTER(CnfInteractionSpec), ctypes.c_int32, _P, _P, _I64, ctypes.c_int32, _P,
                                         _P, _I64, _P]),
  # the kernel Stein discrepancy of x [S, N, D] against the score [S, N, D]: sums [S, 2] doubles, rows [S, N] or NULL,
  # grad_x and grad_s [S, N, D], both or neither
  "cnf_stein_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_stein_splits": (ctypes.c_int, [ctypes.c_int32, _I64, ctypes.c_int32]),
  "cnf_stein": (ctypes.c_int, [ctypes.POINTER(CnfSteinSpec), ctypes.c_int32, _P, _P, _I64, ctypes.c_int32, _P, _P, _P, _P,
                               _P, _I64, _P]),
  # the wild bootstrap of the same statistic: signs [N, P / 32] words, stats [S, P] doubles, raw = q [S, P], t [S] and
  # the diagonal sum [S] doubles, or NULL
  "cnf_stein_boot_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_stein_boot_splits": (ctypes.c_int, [ctypes.c_int32, _I64, ctypes.c_int32]),
  "cnf_stein_boot": (ctypes.c_int, [ctypes.POINTER(CnfSteinSpec), ctypes.c_int32, _P, _P, _I64, ctypes.c_int32, _P,
                                    ctypes.c_int32, _P, _P, _P, _I64, _P]),
  # the kernel density estimate of x [S, N, D] at q [S, Q, D] (NULL: at x itself): log_rho [S, n_bw, Q], score
  # [S, n_bw, Q, D], sums [S, n_bw] doubles, each or NULL
  "cnf_kde_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.POINTER(_I64)]),
  "cnf_kde_splits": (ctypes.c_int, [ctypes.c_int32, _I64, _I64, ctypes.c_int32]),
  "cnf_kde": (ctypes.c_int, [ctypes.POINTER(CnfKdeSpec), ctypes.c_int32, _P, _I64, _P, _I64, ctypes.c_int32, _P, _P, _P, _P,
                             _I64, _P]),
  # the interacting (McKean-Vlasov) particle reference: R replicas of N particles (snap_step: a host array); state
  # [R, N, D], sums [S, R, 3 + D + D D] doubles, pos [S, R, N, D] and hist [S, ny, nx] each or NULL
  "cnf_mv_particles_workspace": (ctypes.c_int, [ctypes.c_int32, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_mv_particles": (ctypes.c_int, [ctypes.POINTER(CnfInteractionSpec), ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.c_float, ctypes.c_double, ctypes.c_double, _I64, ctypes.c_double, _U64, _I64,
                                      ctypes.c_int32, _I64, _P, ctypes.POINTER(_I64), ctypes.c_int32,
                                      ctypes.POINTER(CnfFieldGrid), _P, _P, _P, _P, _P, _I64, _P]),
  # the particle reference of the rwpo problems (centre, times: host arrays): log_h, ess [N], mean_T [N, D], sel [N]
  # int32, and cnf_fp_particles' pos, sums and hist of the bridge's positions, each or NULL
  "cnf_rwpo_particles_workspace": (ctypes.c_int, [_I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64)]),
  "cnf_rwpo_particles": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float] + [ctypes.c_double] * 5
                         + [ctypes.POINTER(ctypes.c_double), _I64, _U64, _I64, _I64, _P, ctypes.POINTER(ctypes.c_double),
                            ctypes.c_int32, ctypes.POINTER(CnfFieldGrid), _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
  "cnf_strerror": (ctypes.c_char_p, [ctypes.c_int]),
  "cnf_build_arch": (ctypes.c_char_p, []),
  "cnf_config_supported": (ctypes.c_int, [_CFG]),
}
# test / measurement knobs: include/cnf_ot_amd_debug.h (not part of the drop-in boundary)
_INTERNAL = {
  "cnf_model_set_fast_math": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_model_set_samples_per_lane": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_model_set_mfma": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_model_set_pwl": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_model_set_dpar": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_model_set_pwl_builder": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_model_last_pwl_builder": (ctypes.c_int, [_P]),
  "cnf_model_set_first_table": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_internal_first_table_floats": (_I64, []),
  "cnf_internal_first_table": (ctypes.c_int, [_P, _P, _P]),
  "cnf_internal_build_tables_into": (ctypes.c_int, [_P, _P, _P, ctypes.c_float, _I64, _P]),
  "cnf_model_set_profiling": (ctypes.c_int, [_P, ctypes.c_int]),
  "cnf_model_read_profile": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
}
PATH_NAMES = {0: "none", 1: "mlp1", 2: "mlp2", 3: "mfma", 4: "tables", 5: "loss_mlp", 6: "loss_tables", 7: "f64", 8: "detect", 9: "dpar", 10: "fields",
              11: "score", 12: "importance"}

_lib = None


class CnfError(RuntimeError):
  def __init__(self, code, where):
    self.code = code
    msg = lib().cnf_strerror(code).decode() if _lib is not None else str(code)
    super().__init__(f"{where}: {msg} ({code})")


def lib():
  """Load the HIP library (once).  Raises if it is absent: no fallback."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise ImportError(
      f"{LIB_PATH} is missing: the cnf_ot_amd product path is hand-written HIP "
      "for gfx950 and has no CPU fallback. Build it with "
      "`python -m cnf_ot_amd.build` (needs hipcc).")
  handle = ctypes.CDLL(LIB_PATH)
  for table in (SYMBOLS, _INTERNAL):
    for name, (res, args) in table.items():
      fn = getattr(handle, name)   # AttributeError if the export is missing
      fn.restype = res
      fn.argtypes = args
  _lib = handle
  return _lib


def check(code, where):
  if code != CNF_OK:
    raise CnfError(code, where)
