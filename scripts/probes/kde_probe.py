"""cnf_kde (the kernel density estimate with its score), value alone and with the score, beside
  (a) its torch composition -- chunked cdist^2, logsumexp, softmax @ x in float32 -- and
  (b) cnf_sinkhorn's pair rate with the map on the same kind of clouds: the same inner loop (a row's online log-sum-exp
      and its weighted column sums), so it is the yardstick.  One iteration: two passes over S (2 N M + N^2 + M^2) pairs,
      the second with the map; N = M = 32 768 at the case's D.
Shapes, S = 9 sets:
  field    Q = 4 096 queries against N = 2^20 sources, D = 2 and 3, one bandwidth
  square   Q = N = 32 768, D = 2 and 10, one and four bandwidths

Timing: HIP events around one call after --warmup rounds; the routes are timed INTERLEAVED (one run of each in turn,
--runs of them) and the medians are reported with min and max.  The composition is chunked over query rows so that a
chunk's [rows, N] matrix stays under --chunk-mb; it is timed on ONE of the nine sets and ONE bandwidth and scaled by
S n_bw (`composed_scaled_from_one_set`).  Pairs: S Q N.  One JSON line per case; --out FILE writes all.

  python scripts/probes/kde_probe.py --out profiles/kde/kde_probe.json
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interaction_probe import interleaved_ms
from sinkhorn_probe import fused_call as sinkhorn_call
from cnf_ot_amd import _capi, utils
from cnf_ot_amd.flows import _stream_ptr

S = 9
CASES = [("field", 4096, 1 << 20, 2, 1), ("field", 4096, 1 << 20, 3, 1),
         ("square", 32768, 32768, 2, 1), ("square", 32768, 32768, 2, 4),
         ("square", 32768, 32768, 10, 1), ("square", 32768, 32768, 10, 4)]          # (name, Q, N, D, n_bw)
YARD_N = 32768


def kde_call(dev, x, q, bws, want_score):
  spec = utils.kde_spec(bws)
  (S_, N, D), Q, B = x.shape, q.shape[1], len(bws)
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_kde_workspace(S_, N, Q, D, B, int(want_score), ctypes.byref(nbytes)), "cnf_kde_workspace")
  ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device=dev)
  lr = torch.empty(S_, B, Q, dtype=torch.float32, device=dev)
  sc = torch.empty(S_, B, Q, D, dtype=torch.float32, device=dev) if want_score else None
  sums = torch.empty(S_, B, dtype=torch.float64, device=dev)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_kde(ctypes.byref(spec), S_, x.data_ptr(), N, q.data_ptr(), Q, D, lr.data_ptr(),
                            None if sc is None else sc.data_ptr(), sums.data_ptr(), ws.data_ptr(), nbytes.value, stream),
                "cnf_kde")
  return run, lr, sc, nbytes.value


def composed_set(x, q, h, rows):
  """(log_rho [Q], score [Q, D]) of ONE set and ONE bandwidth in float32, `rows` queries at a time"""
  N, D = x.shape
  cst = -torch.log(torch.tensor(float(N))) - 0.5 * D * torch.log(torch.tensor(2.0 * torch.pi * h * h))
  lr, sc = [], []
  for i0 in range(0, q.shape[0], rows):
    qi = q[i0:i0 + rows]
    t = torch.cdist(qi, x) ** 2 * (-0.5 / (h * h))
    lr.append(torch.logsumexp(t, 1) + cst.to(t.device))
    sc.append((torch.softmax(t, 1) @ x - qi) / (h * h))
  return torch.cat(lr), torch.cat(sc)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=1)
  ap.add_argument("--chunk-mb", type=int, default=1024)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "kde_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows_out, yard = [], {}
  for name, Q, N, D, B in CASES:
    gen = torch.Generator(device=dev).manual_seed(100 * D + B + len(name))
    x = torch.randn(S, N, D, device=dev, generator=gen)
    q = 1.25 * torch.randn(S, Q, D, device=dev, generator=gen)
    h = utils.kde_bandwidths(x)[0]
    bws = [h] if B == 1 else [0.5 * h, h, 2.0 * h, 4.0 * h]
    if D not in yard:                             # the yardstick: one Sinkhorn iteration with the map at this D
      gy = torch.Generator(device=dev).manual_seed(7 + D)
      ya, yb = torch.randn(S, YARD_N, D, device=dev, generator=gy), 1.25 * torch.randn(S, YARD_N, D, device=dev, generator=gy)
      run_sk = sinkhorn_call(dev, ya, yb, [0.5], True)[0]
      (sk_med, sk_min, sk_max), = interleaved_ms([run_sk], args.runs, args.warmup)
      yard[D] = (sk_med, sk_min, sk_max, 2.0 * S * 4.0 * YARD_N * YARD_N / (sk_med * 1e-3))
      del ya, yb, run_sk
    sk_med, sk_min, sk_max, sk_rate = yard[D]
    value, _, _, _ = kde_call(dev, x, q, bws, False)
    full, lr, sc, ws_bytes = kde_call(dev, x, q, bws, True)
    rows = max(1, min(Q, args.chunk_mb * (1 << 20) // (4 * N * 4)))               # (t, its softmax, cdist and its square)
    comp = lambda: composed_set(x[0], q[0], float(bws[0]), rows)
    (v_med, v_min, v_max), (f_med, f_min, f_max), (c_med, c_min, c_max) = interleaved_ms([value, full, comp], args.runs,
                                                                                           args.warmup)
    c_scale = S * B
    full()
    torch.cuda.synchronize()
    clr, csc = comp()
    pairs = float(S) * Q * N
    row = {"case": name, "S": S, "Q": Q, "N": N, "D": D, "n_bw": B, "runs": args.runs, "bandwidths": [float(b) for b in bws],
           "kde_value_ms": v_med, "kde_value_ms_min": v_min, "kde_value_ms_max": v_max,
           "kde_ms": f_med, "kde_ms_min": f_min, "kde_ms_max": f_max,
           "composed_ms": c_med * c_scale, "composed_ms_min": c_min * c_scale, "composed_ms_max": c_max * c_scale,
           "composed_scaled_from_one_set": True, "composed_chunk_rows": rows, "speedup_over_composed": c_med * c_scale / f_med,
           "pairs": pairs, "kde_value_pairs_per_s": pairs / (v_med * 1e-3), "kde_pairs_per_s": pairs / (f_med * 1e-3),
           "sinkhorn_ms": sk_med, "sinkhorn_ms_min": sk_min, "sinkhorn_ms_max": sk_max, "sinkhorn_pairs_per_s": sk_rate,
           "rate_over_sinkhorn": pairs / (f_med * 1e-3) / sk_rate, "value_rate_over_sinkhorn": pairs / (v_med * 1e-3) / sk_rate,
           "splits": _capi.lib().cnf_kde_splits(S, N, Q, D), "workspace_bytes": ws_bytes,
           "log_rho_abs_diff_set0": float((lr[0, 0] - clr).abs().max()), "score_abs_diff_set0": float((sc[0, 0] - csc).abs().max()),
           "score_abs_max_set0": float(sc[0, 0].abs().max())}
    print(json.dumps(row), flush=True)
    rows_out.append(row)
    del x, q, value, full, lr, sc, clr, csc
    torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
