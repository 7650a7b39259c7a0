"""The C ABI across the translation units of libcnf_ot_amd.so (no GPU needed): every entry point the Python side
binds is exported by the built library and declared in the public header, and the build lists only files that exist."""
import os
import re

from cnf_ot_amd import _capi, build

REPO = os.path.join(os.path.dirname(os.path.abspath(_capi.__file__)), "..")


def test_every_bound_symbol_is_exported_and_declared():
  header = open(os.path.join(REPO, "include", "cnf_ot_amd.h")).read()
  lib = _capi.lib()
  assert len(_capi.SYMBOLS) > 0
  for name in _capi.SYMBOLS:
    assert hasattr(lib, name), f"{name}: not exported by {_capi.LIB_PATH}"
    assert re.search(r"\b" + re.escape(name) + r"\s*\(", header), f"{name}: not declared in include/cnf_ot_amd.h"


def test_the_build_lists_existing_files():
  assert len(set(build.SOURCES)) == len(build.SOURCES) and len(set(build.HEADERS)) == len(build.HEADERS)
  for f in build.SOURCES + build.HEADERS:
    assert os.path.isfile(os.path.join(build.SRC_DIR, f)), f
  on_disk = {f for f in os.listdir(build.SRC_DIR) if f.endswith((".hip", ".h"))}
  listed = {f for f in build.SOURCES + build.HEADERS if os.sep not in f}
  assert on_disk == listed, f"csrc/ and build.py disagree: {sorted(on_disk ^ listed)}"
