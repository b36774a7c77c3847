"""CPU tier: the C-ABI shared library loads and exports every symbol include/seqik.h declares;
argument validation works without a GPU; a missing library fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_PARENT, ROOT, leg_arrays, load_golden


def declared_functions():
    text = open(os.path.join(ROOT, "include", "seqik.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))


def test_header_declares_expected_entry_points():
    assert declared_functions() == sorted(["seqik_abi_version", "seqik_device_count", "seqik_last_error",
                                           "seqik_device_attributes", "seqik_release_workspaces",
                                           "seqik_validate_legs", "seqik_peer_alloc", "seqik_peer_free", "seqik_peer_export",
                                           "seqik_peer_open", "seqik_peer_close", "seqik_peer_copy", "seqik_solve_seq", "seqik_solve_seq_device",
                                           "seqik_head_angles", "seqik_head_angles_device",
                                           "seqik_head_angles_ex", "seqik_head_angles_ex_device", "seqik_signed_angles",
                                           "seqik_validate_legs_generic", "seqik_solve_generic",
                                           "seqik_solve_generic_device",
                                           "seqik_host_alloc", "seqik_host_free", "seqik_host_register",
                                           "seqik_host_unregister", "seqik_frame_chunk_plan", "seqik_selftest_div_sqrt", "seqik_selftest_sqrt_pos",
                                           "seqik_check_faults", "seqik_check_faults_stream", "seqik_stream_open", "seqik_stream_submit",
                                           "seqik_stream_wait", "seqik_stream_reset_carry", "seqik_stream_set_carry", "seqik_stream_close",
                                           "seqik_align_stats_open", "seqik_align_stats_add", "seqik_align_stats_finish",
                                           "seqik_align_stats_reset", "seqik_align_stats_close"])


def test_library_exports_every_declared_symbol(hiplib):
    lib = hiplib.load()
    for name in declared_functions():
        assert hasattr(lib, name), name
    assert sorted(hiplib.EXPORTED_SYMBOLS) == declared_functions()
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION


C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
             "size_t": ctypes.c_size_t}


def header_prototypes(header):
    """{name: (return type, [parameter, ...])} of every ``seqik_*`` prototype of include/<header>, as C text without
    comments and preprocessor lines; ``(void)`` is an empty parameter list."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(seqik_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, name
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def is_pointer_type(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def assert_same_class(c_text, bound, is_parameter, where):
    """``c_text``: a C return type, or a parameter with its name.  Anything with ``*`` matches any ctypes pointer type;
    int, int32_t, int64_t, double and size_t match exactly; a function may return void."""
    if "*" in c_text:
        assert is_pointer_type(bound), (where, c_text, bound)
        return
    words = [w for w in c_text.split() if w != "const"]
    if is_parameter:
        assert len(words) == 2, (where, c_text)   # type and name
    ctype = words[0]
    if ctype == "void" and not is_parameter:
        assert bound is None, (where, c_text, bound)
    else:
        assert ctype in C_SCALARS, (where, c_text)
        assert bound is C_SCALARS[ctype], (where, c_text, bound)


def test_signature_table_matches_the_prototypes(hiplib):
    """Every header's prototypes against ``_lib.SIGNATURES`` -- the table ``load()`` binds the library with: the same
    names per header, the same number of parameters, and the same class for the return value and every parameter."""
    headers = ["seqik.h", "seqik_fk.h", "seqik_frames.h", "seqik_gaps.h", "seqik_resample.h", "seqik_head_align.h"]
    assert sorted(hiplib.SIGNATURES) == sorted(headers)
    lib = hiplib.load()
    n_checked = 0
    for header in headers:
        protos = header_prototypes(header)
        table = {sig[0]: sig[1:] for sig in hiplib.SIGNATURES[header]}
        assert len(table) == len(hiplib.SIGNATURES[header]), header   # no name twice
        assert sorted(table) == sorted(protos), header
        for name, (ret, params) in protos.items():
            restype, argtypes = table[name][0], list(table[name][1:])
            assert len(argtypes) == len(params), (name, params, argtypes)
            assert_same_class(ret, restype, False, name)
            for p, a in zip(params, argtypes):
                assert_same_class(p, a, True, name)
            # ... and it is what the loaded library is bound with ((void) -> argtypes == [], not unset)
            fn = getattr(lib, name)
            assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == argtypes, name
            n_checked += 1
    assert n_checked == 60
    # the parser sees what it should: a known prototype, in full
    assert header_prototypes("seqik_resample.h")["seqik_resample_count"] == \
        ("int64_t", ["int64_t n_frames", "double original_ts", "double new_ts"])
    assert header_prototypes("seqik.h")["seqik_abi_version"] == ("int", [])
    # the per-header name lists are the table's
    for header, names in (("seqik.h", hiplib.EXPORTED_SYMBOLS), ("seqik_fk.h", hiplib.FK_EXPORTED_SYMBOLS),
                          ("seqik_frames.h", hiplib.FRAMES_EXPORTED_SYMBOLS), ("seqik_gaps.h", hiplib.GAPS_EXPORTED_SYMBOLS),
                          ("seqik_resample.h", hiplib.RESAMPLE_EXPORTED_SYMBOLS),
                          ("seqik_head_align.h", hiplib.HEAD_ALIGN_EXPORTED_SYMBOLS)):
        assert names == [sig[0] for sig in hiplib.SIGNATURES[header]]


def test_struct_layout_matches_header(hiplib):
    assert ctypes.sizeof(hiplib.SeqikLegParams) == 8 * (4 + 14 + 27)
    assert ctypes.sizeof(hiplib.SeqikOptions) == 88  # ABI 3: + chunk_flags, chunk_states, chunk_resume
    assert hiplib.SeqikOptions.frame_chunk.offset == 32 and hiplib.SeqikOptions.chunk_tol.offset == 40
    assert hiplib.SeqikOptions.frame_lead.offset == 52 and hiplib.SeqikOptions.chunk_stats.offset == 56
    assert hiplib.SeqikOptions.chunk_flags.offset == 64 and hiplib.SeqikOptions.chunk_states.offset == 72
    assert hiplib.SeqikOptions.chunk_resume.offset == 80
    assert ctypes.sizeof(hiplib.SeqikLayout) == 48 and ctypes.sizeof(hiplib.SeqikAffine) == 56


def test_validate_legs_error_codes(hiplib):
    z = load_golden("df3d_100")
    _, seg, b, seeds = leg_arrays(z, "RF")
    good = hiplib.leg_params_from_arrays(seg, b, seeds)
    hiplib.validate_legs([good])
    bad_seed = seeds.copy()
    bad_seed[1] = 4.0
    with pytest.raises(ValueError, match="Initial guess is outside of provided bounds"):
        hiplib.validate_legs([hiplib.leg_params_from_arrays(seg, b, bad_seed)])
    hiplib.validate_legs([hiplib.leg_params_from_arrays(seg, b, bad_seed)], 2, 4)  # stage 1 not run: not checked
    bb = b.copy()
    bb[2] = (1.0, -1.0)
    with pytest.raises(ValueError, match="strictly less"):
        hiplib.validate_legs([hiplib.leg_params_from_arrays(seg, bb, seeds)])
    with pytest.raises(ValueError, match="Maximum stage number is 4"):
        hiplib.validate_legs([good], 2, 5)
    # floating-point contract (csrc/seqik_core.hpp): a limit of exactly 0 is served (the shipped tables have three), a
    # non-zero limit below 2^-600 in magnitude is refused
    tiny = b.copy()
    tiny[3] = (tiny[3][0], 1e-250)
    with pytest.raises(ValueError, match="smaller than 2\\^-600"):
        hiplib.validate_legs([hiplib.leg_params_from_arrays(seg, tiny, seeds)])
    assert any(0.0 in (lo, hi) for lo, hi in b)


def test_solve_rejects_bad_arguments_before_touching_the_gpu(hiplib):
    z = load_golden("df3d_100")
    pose, seg, b, seeds = leg_arrays(z, "RF")
    lp = hiplib.leg_params_from_arrays(seg, b, seeds)
    with pytest.raises(ValueError):
        hiplib.solve_seq(pose[None, None, :4], [lp], 3, 2)
    with pytest.raises(ValueError):
        hiplib.solve_seq(pose[:4], [lp])  # wrong rank
    bad = seeds.copy()
    bad[26] = 9.0  # claw seed outside +-pi
    with pytest.raises(ValueError, match="outside of provided bounds"):
        hiplib.solve_seq(pose[None, None, :4], [hiplib.leg_params_from_arrays(seg, b, bad)])


def test_non_finite_key_points_raise_like_scipy(hiplib):
    z = load_golden("df3d_100")
    pose, seg, b, seeds = leg_arrays(z, "RF")
    bad = pose[None, None, :8].copy()
    bad[0, 0, 3, 2, 1] = np.nan
    with pytest.raises(ValueError, match="Residuals are not finite"):
        hiplib.solve_seq(bad, [hiplib.leg_params_from_arrays(seg, b, seeds)])
    with pytest.raises(ValueError, match="Residuals are not finite"):
        hiplib.solve_generic(bad, [hiplib.leg_params_from_arrays(seg, b, seeds)])


def test_missing_library_fails_loudly():
    code = ("import sys; sys.path.insert(0, %r); from seqikpy_amd import _lib\n"
            "try:\n    _lib.load()\nexcept _lib.SeqikLibraryError as e:\n    print('LOUD', e)\n" % PKG_PARENT)
    env = dict(os.environ, SEQIK_LIB="/nonexistent/libseqik_hip.so")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "LOUD" in out.stdout and "no CPU fallback" in out.stdout, out.stdout + out.stderr


def test_product_does_not_import_the_oracle():
    """The package must not reach into oracle/ (it is test infrastructure)."""
    pkg = os.path.join(PKG_PARENT, "seqikpy_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            for needle in ("import oracle", "from oracle", "c_oracle", "ref_import", "libseqik_oracle"):
                assert needle not in src, (fn, needle)
    csrc = os.path.join(PKG_PARENT, "csrc")
    for fn in os.listdir(csrc):
        if fn.endswith((".hip", ".hpp", ".h", ".cpp")):
            for line in open(os.path.join(csrc, fn)):
                if line.lstrip().startswith("#include"):
                    assert "oracle" not in line, (fn, line)


def test_committed_pmc_summary_belongs_to_these_kernel_sources(hiplib):
    """bench.py prices its roofline with the PMC counters of profiles/traffic_r06*.json only while they were measured on
    the kernel code of this tree (`_lib.csrc_sha256`: code only, comments and white space do not count).  If this fails the
    solver kernels changed: re-run `bash scripts/gpu_profile.sh r06` / `r06s --variant smooth` + `scripts/summarize_profile.py r06 r06` / `r06s r06`
    (and `bash scripts/gpu_latency_profile.sh r06` + `scripts/latency_floor.py r06 r06` for the latency-bound kernels)."""
    import json
    assert hiplib._code_only("a = b; // note\n/* block\n comment */  c  =\td;") == "a = b; c = d;"
    for name in ("traffic_r06.json", "traffic_r06_smooth.json"):
        t = json.load(open(os.path.join(ROOT, "profiles", name)))
        assert t["csrc_files"] == hiplib.KERNEL_SOURCES
        assert t["csrc_sha256"] == hiplib.csrc_sha256(), name
    lat = json.load(open(os.path.join(ROOT, "profiles", "r06_latency_floor.json")))
    assert lat["csrc_files"] == hiplib.LATENCY_SOURCES and lat["csrc_sha256"] == hiplib.csrc_sha256(hiplib.LATENCY_SOURCES)
