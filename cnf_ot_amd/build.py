"""Builds cnf_ot_amd/lib/libcnf_ot_amd.so for gfx950 with hipcc (in-tree).

hipcc cross-compiles without a GPU; the resulting .so travels to the GPU box
with the repo snapshot.  ``python -m cnf_ot_amd.build`` or
``__graft_entry__.build()``.
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SRC_DIR = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libcnf_ot_amd.so")
OBJ_DIR = os.path.join(LIB_DIR, "obj")                     # one object per source; FLAGS: what they were compiled with
# (the longest compile first: it bounds the build)
SOURCES = ["cnf_flow.hip", "cnf_grad.hip", "cnf_grad_pwl.hip", "cnf_importance.hip", "cnf_mmd.hip", "cnf_mmd_perm.hip", "cnf_knn.hip", "cnf_interaction.hip", "cnf_interaction_vjp.hip", "cnf_stein.hip", "cnf_stein_boot.hip", "cnf_kde.hip", "cnf_hopf_cole.hip", "cnf_fp_particles.hip", "cnf_fp_grid.hip",
           "cnf_mv_particles.hip", "cnf_rwpo_particles.hip", "cnf_sinkhorn.hip", "cnf_sliced.hip", "cnf_step.hip", "cnf_model.hip", "cnf_rng.hip"]
HEADERS = ["cnf_device.h", "cnf_terms.h", "cnf_common.h", "cnf_host.h", "cnf_flow_tile.h", "cnf_backward.h", "cnf_pwl.h",
           "cnf_pwl_build.h", "cnf_first_table.h", "cnf_fp_stats.h", "cnf_pairs.h", "cnf_interaction_pairs.h", os.path.join("..", "..", "include", "cnf_ot_amd.h")]
VARIANT_PATH = os.path.join(LIB_DIR, "BUILD_VARIANT")     # "full" or "minimal": what the .so in tree contains
ARCH = "gfx950"


def _hipcc():
  for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
    if cand and os.path.exists(cand):
      return cand
  raise RuntimeError("hipcc not found (need ROCm's hipcc to build the gfx950 kernels)")


def _variant() -> str:
  try:
    with open(VARIANT_PATH) as f:
      return f.read().strip()
  except OSError:
    return ""


def is_stale(minimal: bool = False) -> bool:
  if not os.path.exists(LIB_PATH):
    return True
  if not minimal and _variant() != "full":     # a quick-iteration build must never pass for the full one
    return True
  t = os.path.getmtime(LIB_PATH)
  deps = [os.path.join(SRC_DIR, f) for f in SOURCES + HEADERS]
  return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _jobs() -> int:
  """hipcc processes at a time: MAX_JOBS if set, never more than one per source or 16."""
  try:
    n = int(os.environ.get("MAX_JOBS", ""))
  except ValueError:
    n = 16
  return max(1, min(n, len(SOURCES), 16))


def build(force: bool = False, minimal: bool = False, verbose: bool = False) -> str:
  """Compile every HIP source to an object, side by side, and link them into one shared library.  `minimal` builds
  only the default (hidden_size=16, num_bins=5) kernels -- for quick iteration."""
  if not force and not is_stale(minimal):
    return LIB_PATH
  os.makedirs(OBJ_DIR, exist_ok=True)
  hipcc = _hipcc()
  flags = ["-O3", f"--offload-arch={ARCH}", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
  if minimal:
    flags.append("-DCNF_MINIMAL_CONFIGS")
  flags += os.environ.get("CNF_EXTRA_FLAGS", "").split()    # experiment switches (scripts/): never set by the product
  # An object is kept while it is newer than its source and every header and was compiled with these flags
  flags_path = os.path.join(OBJ_DIR, "FLAGS")
  try:
    with open(flags_path) as f:
      same_flags = f.read() == " ".join(flags)
  except OSError:
    same_flags = False
  newest_header = max(os.path.getmtime(os.path.join(SRC_DIR, h)) for h in HEADERS)

  def compile_one(name):
    src, obj = os.path.join(SRC_DIR, name), os.path.join(OBJ_DIR, os.path.splitext(name)[0] + ".o")
    if not force and same_flags and os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(src), newest_header):
      return obj
    cmd = [hipcc, *flags, "-c", src, "-o", obj]
    if verbose:
      print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
      raise RuntimeError(f"hipcc failed on {name}:\n" + res.stdout + res.stderr)
    return obj

  if os.path.exists(flags_path):
    os.remove(flags_path)                                   # (an interrupted build leaves no claim about its objects)
  with ThreadPoolExecutor(max_workers=_jobs()) as pool:
    objs = list(pool.map(compile_one, SOURCES))
  with open(flags_path, "w") as f:
    f.write(" ".join(flags))
  tmp = LIB_PATH + ".tmp"
  cmd = [hipcc, f"--offload-arch={ARCH}", "-fPIC", "-shared", *objs, "-o", tmp]
  if verbose:
    print(" ".join(cmd), flush=True)
  res = subprocess.run(cmd, capture_output=True, text=True)
  if res.returncode != 0:
    raise RuntimeError("hipcc failed to link:\n" + res.stdout + res.stderr)
  os.replace(tmp, LIB_PATH)
  with open(VARIANT_PATH, "w") as f:
    f.write("minimal\n" if minimal else "full\n")
  return LIB_PATH


if __name__ == "__main__":
  path = build(force="--force" in sys.argv, minimal="--minimal" in sys.argv, verbose=True)
  print("built", path)
