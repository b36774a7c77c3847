"""The scaffolding the bit-for-bit tests stand on is itself sound: the shared assertion (tests/pass_cut_support.py) fails on
a reference that differs in one ulp, and the harness builder (tests/harness_build.py) sees a header of a header."""
import os
import shutil

import numpy as np
import pytest

import harness_build
from pass_cut_support import LAUNCH_PATHS, assert_equal_reference


def _synthetic(rng):
    S, L, N = 3, 2, 4
    return dict(angles=rng.normal(0.0, 1.0, (S, L, N, 7)), fk=rng.normal(0.0, 1.0, (S, L, N, 9, 3)),
                status=rng.integers(1, 5, (S, L, N, 4)).astype(np.int32), nfev=rng.integers(1, 30, (S, L, N, 4)).astype(np.int32))


def _one_ulp(a):
    a = a.copy()
    a[1, 1, 2, 3] = np.nextafter(a[1, 1, 2, 3], np.inf)
    return a


def test_shared_assertion_fails_on_a_differing_reference():
    ref = _synthetic(np.random.default_rng(4))
    n_chains = 3 * 2

    def out(**changed):
        return {**{k: v.copy() for k, v in ref.items()}, "chunk_stats": dict(chunks=2 * n_chains), **changed}

    changed_status, changed_nfev = ref["status"].copy(), ref["nfev"].copy()
    changed_status[2, 0, 1, 3] += 1
    changed_nfev[0, 1, 3, 0] += 1
    for path in LAUNCH_PATHS:
        outs = [out()] * (3 if path == "subset" else 1)
        assert_equal_reference(outs, ref, path, n_chains)
        for key in ("angles", "fk"):
            with pytest.raises(AssertionError):
                assert_equal_reference(outs[:-1] + [out(**{key: _one_ulp(ref[key])})], ref, path, n_chains)
        for changed in (dict(status=changed_status), dict(nfev=changed_nfev)):
            if path == "staged_diag":
                with pytest.raises(AssertionError):
                    assert_equal_reference([out(**changed)], ref, path, n_chains)
            else:   # the other paths do not report them
                assert_equal_reference(outs[:-1] + [out(**changed)], ref, path, n_chains)
    for chunks in (2 * n_chains - 1, 2 * n_chains + 1, n_chains):
        with pytest.raises(AssertionError):
            assert_equal_reference([out(chunk_stats=dict(chunks=chunks))], ref, "chunked", n_chains)
    # a NaN is no wildcard: the comparison is on the words
    with pytest.raises(AssertionError):
        bad = ref["angles"].copy()
        bad[0, 0, 0, 0] = np.nan
        assert_equal_reference([out(angles=bad)], ref, "fused", n_chains)


def test_builder_sees_a_transitive_header(tmp_path, monkeypatch):
    top, tmp_path = tmp_path, tmp_path / "tree"
    tmp_path.mkdir()
    (tmp_path / "second.h").write_text("#define ANSWER 42\n")
    (tmp_path / "first.h").write_text('#include "second.h"\n')
    src = tmp_path / "probe.hip"
    src.write_text('#include "first.h"\nextern "C" int answer() { return ANSWER; }\n')
    out_dir = str(tmp_path / "_build")
    compiles = []
    check_call = harness_build.subprocess.check_call
    monkeypatch.setattr(harness_build.subprocess, "check_call", lambda cmd, *a, **k: (compiles.append(cmd), check_call(cmd, *a, **k)))

    with monkeypatch.context() as m:
        m.setattr(harness_build, "find_hipcc", lambda: None)
        with pytest.raises(pytest.skip.Exception, match="hipcc not available"):
            harness_build.build_harness(str(src), out_dir)
    assert not compiles and not os.path.exists(out_dir)

    so = harness_build.build_harness(str(src), out_dir)   # (skips here without hipcc)
    assert so == os.path.join(out_dir, "libprobe.so") and os.path.exists(so) and len(compiles) == 1
    assert all(flag in compiles[0] for flag in harness_build.FLAGS)
    assert {"-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared"} < set(harness_build.FLAGS)   # (and host only)
    with open(so + ".d") as f:
        deps = harness_build.depfile_paths(f.read())
    assert {str(src), str(tmp_path / "first.h"), str(tmp_path / "second.h")} <= set(deps)
    assert sorted(os.listdir(out_dir)) == ["libprobe.so", "libprobe.so.d"]   # no temporary left behind

    assert harness_build.build_harness(str(src), out_dir) == so and len(compiles) == 1   # twice: one compile

    ahead = os.path.getmtime(so) + 10.0
    os.utime(tmp_path / "second.h", (ahead, ahead))
    harness_build.build_harness(str(src), out_dir)
    assert len(compiles) == 2
    os.utime(tmp_path / "second.h", (ahead - 20.0, ahead - 20.0))
    harness_build.build_harness(str(src), out_dir)
    assert len(compiles) == 2

    os.remove(so + ".d")
    harness_build.build_harness(str(src), out_dir)
    assert len(compiles) == 3 and os.path.exists(so + ".d")

    with open(so + ".d") as f:   # (a _build/ from another machine names paths that are not here)
        rule = f.read()
    with open(so + ".d", "w") as f:
        f.write(rule.rstrip("\n") + " \\\n  /nowhere/on/this/machine/seqik.h\n")
    assert "/nowhere/on/this/machine/seqik.h" in harness_build.depfile_paths(open(so + ".d").read())
    harness_build.build_harness(str(src), out_dir)
    assert len(compiles) == 4
    harness_build.build_harness(str(src), out_dir)
    assert len(compiles) == 4

    # a copy of the tree with its _build/: the copied depfile is about the other tree's files
    shutil.copytree(tmp_path, top / "copy")
    so2 = harness_build.build_harness(str(top / "copy" / "probe.hip"), str(top / "copy" / "_build"))
    assert len(compiles) == 5
    with open(so2 + ".d") as f:
        assert str(top / "copy" / "second.h") in harness_build.depfile_paths(f.read())
    harness_build.build_harness(str(top / "copy" / "probe.hip"), str(top / "copy" / "_build"))
    assert len(compiles) == 5

    # a compile that fails leaves the library that was there, and nothing else
    before = os.path.getmtime(so)
    (tmp_path / "second.h").write_text("#error broken\n")
    os.utime(tmp_path / "second.h", (before + 10.0, before + 10.0))
    with pytest.raises(harness_build.subprocess.CalledProcessError):
        harness_build.build_harness(str(src), out_dir)
    assert os.path.getmtime(so) == before and sorted(os.listdir(out_dir)) == ["libprobe.so", "libprobe.so.d"]

