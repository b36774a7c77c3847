"""TEST INFRASTRUCTURE -- the one way a host harness (tests/harness/*.hip: device code compiled for the host so that the
CPU tier can compare it bit for bit) is built.  The flags are fixed: the results are compared as integers, so -O2 and
-ffp-contract=off must not move.  What a library depends on comes from the compiler's own depfile, never from a list: a
library is rebuilt when it or its depfile is missing, when a file the depfile names is newer than it or is not there, or
when the depfile is not about this source (a _build/ that came with a copy of the tree names the other tree's files)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

FLAGS = ("--offload-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared")
BUILD_DIR = os.path.join(ROOT, "tests", "harness", "_build")


def find_hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return hipcc if os.path.exists(hipcc) else None


def depfile_paths(text):
    """The prerequisites of the make rule the compiler writes: `target: dep dep \\<newline> dep ...`, a space inside a
    path written as `\\ `."""
    rule = text.replace("\\\n", " ").split(": ", 1)
    if len(rule) != 2:
        return []
    return [p.replace("\\ ", " ") for p in re.split(r"(?<!\\)\s+", rule[1].strip()) if p]


def is_stale(so, src):
    try:
        built = os.path.getmtime(so)
        with open(so + ".d") as f:
            deps = depfile_paths(f.read())
        return src not in deps or any(os.path.getmtime(d) > built for d in deps)
    except OSError:   # no library, no depfile, or a file the depfile names is not there
        return True


def build_harness(src, out_dir=None, extra_flags=()):
    """Compiles `src` for the host into `out_dir`/lib<name>.so if that library is stale -> its path.  Skips the calling
    test when there is no hipcc."""
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    src = os.path.abspath(src)   # (the depfile then holds absolute paths)
    out_dir = out_dir or BUILD_DIR
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "lib" + os.path.splitext(os.path.basename(src))[0] + ".so")
    if is_stale(so, src):
        # to a temporary name, then onto the library: an interrupted compile leaves nothing that loads
        tmp = f"{so}.tmp{os.getpid()}"
        try:
            subprocess.check_call([hipcc, *FLAGS, *extra_flags, "-MMD", "-MF", tmp + ".d", "-MT", so, "-o", tmp, src])
            os.replace(tmp + ".d", so + ".d")
            os.replace(tmp, so)
        finally:
            for leftover in (tmp, tmp + ".d"):
                if os.path.exists(leftover):
                    os.remove(leftover)
    return so
