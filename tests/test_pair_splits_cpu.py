"""The column splits of the six pair units against ONE statement of the rule (csrc/cnf_pairs.h: pair_splits).  For a pass
of `base` workgroups per split over `tiles` tiles of 64 columns
  want = ceil(2048 / base),  most = max(1, min(want, tiles, 64)),  per = ceil(tiles / most),  P = ceil(tiles / per)
and a unit supplies its own base and tiles (rg(n): n's row groups of 512 rows, a workgroup's 256 lanes at two rows each):
  cnf_mmd          S (2 rg(N) + rg(M)),  the tiles of max(N, M)
  cnf_knn          S blocks rg(N) (blocks = 2 with a second set, else 1),  the tiles of max(N, M)
  cnf_sinkhorn     2 S (rg(N) + rg(M)),  the tiles of max(N, M)
  cnf_interaction  S rg(rows) (rows = Q in query mode, else N),  the tiles of N
  cnf_stein        S rg_D(N) (two rows per lane up to D = 8, one above),  the tiles of N
  cnf_kde          S rg(Q) (counted at two rows per lane whatever D and the bandwidths take),  the tiles of N
No GPU: the queries are host arithmetic.  Every point also shows that no split is empty and that 1 <= P <= 64.
"""
import itertools

TARGET_WGS, TILE, MAX_SPLIT, LANES = 2048, 64, 64, 256
SETS = (1, 2, 9, 64)
SIZES = (2, 64, 65, 511, 512, 513, 4096, 32768, 1 << 20)       # the edges of the rule: a tile, a row group, the limit
DIMS = (1, 8, 9, 14)                                           # (cnf_stein's rows per lane change between 8 and 9)


def _ceil(a, b):
  return -(-a // b)


def _rule(base, tiles):
  """(P, tiles per split) of the one rule"""
  want = _ceil(TARGET_WGS, base)
  most = max(1, min(want, tiles, MAX_SPLIT))
  per = _ceil(tiles, most)
  return _ceil(tiles, per), per


def _rg(n, rows_per_lane=2):
  return _ceil(n, LANES * rows_per_lane)


def _check(got, base, n_col, where):
  tiles = _ceil(n_col, TILE)
  P, per = _rule(base, tiles)
  assert got == P, (where, got, P)
  assert 1 <= P <= MAX_SPLIT and (P - 1) * per < tiles, (where, P, per, tiles)     # in range, and no split is empty


def test_two_set_units_follow_the_one_rule():
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  for S, N, M in itertools.product(SETS, SIZES, SIZES):
    for D in (1, 14):                                          # (the count does not depend on D)
      longer = max(N, M)
      _check(lib.cnf_mmd_splits(S, N, M, D), S * (2 * _rg(N) + _rg(M)), longer, ("mmd", S, N, M, D))
      _check(lib.cnf_sinkhorn_splits(S, N, M, D), 2 * S * (_rg(N) + _rg(M)), longer, ("sinkhorn", S, N, M, D))
      _check(lib.cnf_knn_splits(S, N, M, D), S * 2 * _rg(N), longer, ("knn", S, N, M, D))
  for S, N, D in itertools.product(SETS, SIZES, (1, 14)):
    _check(lib.cnf_knn_splits(S, N, 0, D), S * _rg(N), N, ("knn, one set", S, N, D))
    _check(lib.cnf_knn_splits(S, N, 1, D), S * 2 * _rg(N), N, ("knn, M = 1", S, N, D))
  for S, N in itertools.product(SETS, (2, 65, 1 << 20, 1 << 24)):            # cnf_mmd alone takes sets of 2^24 points
    _check(lib.cnf_mmd_splits(S, 1 << 24, N, 2), S * (2 * _rg(1 << 24) + _rg(N)), 1 << 24, ("mmd", S, 1 << 24, N))
    _check(lib.cnf_mmd_splits(S, N, 1 << 24, 2), S * (2 * _rg(N) + _rg(1 << 24)), 1 << 24, ("mmd", S, N, 1 << 24))


def test_one_set_units_follow_the_one_rule():
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  for S, N, D in itertools.product(SETS, SIZES, DIMS):
    _check(lib.cnf_interaction_splits(S, N, 0, D), S * _rg(N), N, ("interaction, self", S, N, D))
    _check(lib.cnf_stein_splits(S, N, D), S * _rg(N, 2 if D <= 8 else 1), N, ("stein", S, N, D))
  for S, N, Q in itertools.product(SETS, SIZES, (1,) + SIZES):
    for D in (1, 14):
      _check(lib.cnf_interaction_splits(S, N, Q, D), S * _rg(Q), N, ("interaction, query", S, N, Q, D))
      _check(lib.cnf_kde_splits(S, N, Q, D), S * _rg(Q), N, ("kde", S, N, Q, D))
  for S, Q in itertools.product(SETS, (1,) + SIZES):                         # cnf_kde alone takes one source
    _check(lib.cnf_kde_splits(S, 1, Q, 3), S * _rg(Q), 1, ("kde, N = 1", S, Q))
