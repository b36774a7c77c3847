"""Skip mode on streams (include/seqik_stream_gaps.h, csrc/seqik_stream.hip, seqikpy_amd/streaming.py).

CPU tier: the header and exports, the seed state (bit-equivalent to no init_angles on the host-run device core), the
carried contract walked slab by slab on the host (compact -> solve from the state -> carry rule -> expand == the solver
on the recording with the missing frames deleted), argument handling.  GPU tier (`-m gpu`): skip streams against
`_lib.solve_seq(..., missing="skip")` / `_lib.solve_generic(..., missing="skip")` of the unsplit input -- slabs of
sequences, carried time slabs (serial and chunked), the generic chain, the fused alignment, and the carry controls.
Everything is compared bit for bit; NaN exactly at the missing leg-frames."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, leg_arrays, load_golden
from gaps_model import load_gaps_harness, np_missing
from stream_gaps_model import (frames, load_stream_gaps_harness, mark, np_next_state, np_next_state_batch,
                               np_seed_state)
from test_capi_symbols import assert_same_class, header_prototypes

STREAM_GAPS_SYMBOLS = ["seqik_stream_open_skip", "seqik_stream_seed_state", "seqik_stream_get_carry"]
NON_FINITE = (np.nan, np.inf, -np.inf)
MISSING = -100


@pytest.fixture(scope="module")
def gaps_harness():
    h = load_gaps_harness()
    if h is None:
        pytest.skip("hipcc not available")
    return h


@pytest.fixture(scope="module")
def carry_harness():
    h = load_stream_gaps_harness()
    if h is None:
        pytest.skip("hipcc not available")
    return h


def _params(lib, z, legs):
    return [lib.leg_params_from_arrays(z[f"{l}_seg"], z[f"{l}_bounds"], z[f"{l}_seeds"]) for l in legs]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def assert_nan_exactly_at(out, miss, what=""):
    """angles (..., N, 7) and fk (..., N, 9, 3) or None: every value of a missing leg-frame is NaN, none of the others."""
    a = np.isnan(out["angles"])
    assert np.array_equal(a.all(axis=-1), miss) and np.array_equal(a.any(axis=-1), miss), what
    if out.get("fk") is not None:
        f = np.isnan(out["fk"])
        assert np.array_equal(f.all(axis=(-1, -2)), miss) and np.array_equal(f.any(axis=(-1, -2)), miss), what


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_three_entry_points_and_load_binds_them(hiplib):
    text = open(os.path.join(ROOT, "include", "seqik_stream_gaps.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(STREAM_GAPS_SYMBOLS)
    assert sorted(hiplib.STREAM_GAPS_SIGNATURES) == ["seqik_stream_gaps.h"]
    assert hiplib.STREAM_GAPS_EXPORTED_SYMBOLS == [s[0] for s in hiplib.STREAM_GAPS_SIGNATURES["seqik_stream_gaps.h"]]
    assert sorted(hiplib.STREAM_GAPS_EXPORTED_SYMBOLS) == declared
    others = [hiplib.EXPORTED_SYMBOLS, hiplib.FK_EXPORTED_SYMBOLS, hiplib.FRAMES_EXPORTED_SYMBOLS,
              hiplib.GAPS_EXPORTED_SYMBOLS, hiplib.RESAMPLE_EXPORTED_SYMBOLS, hiplib.RESAMPLE_DER_EXPORTED_SYMBOLS,
              hiplib.HEAD_ALIGN_EXPORTED_SYMBOLS]
    for names in others:
        assert not set(declared) & set(names)
    # neither of the pinned tables gained the header
    assert "seqik_stream_gaps.h" not in hiplib.SIGNATURES and "seqik_stream_gaps.h" not in hiplib.EXTENSION_SIGNATURES
    for header in ("seqik.h", "seqik_gaps.h"):
        assert not set(declared) & set(header_prototypes(header))
    protos = header_prototypes("seqik_stream_gaps.h")
    table = {sig[0]: sig[1:] for sig in hiplib.STREAM_GAPS_SIGNATURES["seqik_stream_gaps.h"]}
    assert sorted(table) == sorted(protos) == declared
    lib = hiplib.load()
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name][0], list(table[name][1:])
        assert len(argtypes) == len(params), (name, params, argtypes)
        assert_same_class(ret, restype, False, name)
        for p, a in zip(params, argtypes):
            assert_same_class(p, a, True, name)
        fn = getattr(lib, name)             # the library exports it and load() bound it with the table's row
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the skip open takes exactly what the plain open takes
    assert protos["seqik_stream_open_skip"] == header_prototypes("seqik.h")["seqik_stream_open"]
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_stream_gaps.h" in open(os.path.join(ROOT, "setup.py")).read()
    assert "seqik_stream_gaps.h" in open(os.path.join(ROOT, "include", "seqik_gaps.h")).read()


def test_seed_state_is_the_stages_start_values(hiplib, carry_harness):
    z = load_golden("df3d_100")
    legs = [str(l) for l in z["legs"]]
    state = hiplib.stream_seed_state(_params(hiplib, z, legs))
    assert state.shape == (6, 7)
    for li, leg in enumerate(legs):
        seeds = z[f"{leg}_seeds"]
        assert np.array_equal(state[li], seeds[[1, 2, 7, 8, 15, 16, 25]]), leg
        assert np.array_equal(state[li], np_seed_state(seeds)) and np.array_equal(state[li], carry_harness.seed_state(seeds))
    zg = load_golden("generic_rf_100")
    glegs = [str(l) for l in zg["legs"]]
    gstate = hiplib.stream_seed_state(_params(hiplib, zg, glegs), generic=True)
    link_dof = [2, 0, 1, 3, 4, 5, 6]        # kGenericLinkDof
    for li, leg in enumerate(glegs):
        seeds = zg[f"{leg}_seeds"]
        for i in range(7):
            assert gstate[li, link_dof[i]] == seeds[19 + i], (leg, i)
        assert np.array_equal(gstate[li], np_seed_state(seeds, True))
        assert np.array_equal(gstate[li], carry_harness.seed_state(seeds, True))
    # the two chain kinds really differ (a generic stream fed the sequential mapping would start elsewhere)
    distinct = np.arange(27, dtype=np.float64)
    assert not np.array_equal(np_seed_state(distinct), np_seed_state(distinct, True))
    lib = hiplib.load()
    assert lib.seqik_stream_seed_state(None, 1, 0, None) == hiplib.ERR_ARG


def test_seed_state_equals_no_init_on_the_host_run_core(host_harness):
    z = load_golden("df3d_100")
    for leg in ["RF", "LH", "RM"]:
        pose, seg, b, seeds = leg_arrays(z, leg)
        a = host_harness.run(pose, seg, b, seeds, init=None)
        c = host_harness.run(pose, seg, b, seeds, init=np_seed_state(seeds))
        for k in ("angles", "fk", "status", "nfev"):
            assert np.array_equal(a[k], c[k]), (leg, k)
    zg = load_golden("generic_rf_100")
    pose, seg, b, seeds = leg_arrays(zg, "RF")
    a = host_harness.run_generic(pose, seg, b, seeds, init=None)
    c = host_harness.run_generic(pose, seg, b, seeds, init=np_seed_state(seeds, True))
    for k in ("angles", "fk", "status", "nfev"):
        assert np.array_equal(a[k], c[k]), k


def test_carry_rule_on_the_host(carry_harness):
    assert [carry_harness.carry_slot(n) for n in (0, 1, 2, 16, 2 ** 31 - 1)] == [-1, 0, 1, 15, 2 ** 31 - 2]
    rng = np.random.default_rng(1)
    cang = rng.normal(size=(16, 7))
    state = rng.normal(size=7)
    assert np.array_equal(carry_harness.carry(cang, 0, state), state)
    for nv in (1, 7, 16):
        assert np.array_equal(carry_harness.carry(cang, nv, state), cang[nv - 1])


def _host_patterns(n, rng):
    """The two gap patterns of the host walk (slabs of 16 frames)."""
    return {"blocks_and_random": frames(n, (0, 23), (48, 64)) | (rng.random(n) < 0.3),
            "last_frame_of_slabs": frames(n, 15, 31, (76, 80), 95, n - 1)}


def test_carried_contract_on_the_host(host_harness, gaps_harness, carry_harness):
    """Slab by slab on the host: compact and pad -> the solver's device code from `state` -> the carry rule -> expand.
    The non-missing frames reproduce the solve of the recording with the missing frames deleted bit for bit, and the
    state after every slab is the model's: the angles at the chain's last non-missing frame so far, else the seed state."""
    z = load_golden("df3d_100")
    T = 16
    for leg in ["RF", "LH", "RM"]:
        pose, seg, b, seeds = leg_arrays(z, leg)
        n = pose.shape[0]
        rng = np.random.default_rng(17)
        for name, miss in _host_patterns(n, rng).items():
            gp = mark(pose, miss, rng, values=NON_FINITE)
            assert np.array_equal(np_missing(gp), miss)
            state = np_seed_state(seeds)
            model_state = state.copy()
            out = dict(angles=np.empty((n, 7)), fk=np.empty((n, 9, 3)), status=np.empty((n, 4), np.int32),
                       nfev=np.empty((n, 4), np.int32))
            for t0 in range(0, n, T):
                sl = slice(t0, min(n, t0 + T))
                cpose, mp, nv = gaps_harness.compact(gp[sl], seg)
                assert nv == (~miss[sl]).sum()
                solved = host_harness.run(cpose, seg, b, seeds, init=state)
                state = carry_harness.carry(solved["angles"], nv, state)
                out["angles"][sl] = gaps_harness.expand(mp, solved["angles"])
                out["fk"][sl] = gaps_harness.expand(mp, solved["fk"])
                out["status"][sl] = gaps_harness.expand(mp, solved["status"], MISSING)
                out["nfev"][sl] = gaps_harness.expand(mp, solved["nfev"], 0)
                model_state = np_next_state(out["angles"][sl], model_state)
                assert np.array_equal(state, model_state), (leg, name, t0)
                if miss[:sl.stop].all():
                    assert np.array_equal(state, np_seed_state(seeds)), (leg, name, t0)
            ref = host_harness.run(gp[~miss], seg, b, seeds)
            for k in ("angles", "fk", "status", "nfev"):
                assert np.array_equal(out[k][~miss], ref[k]), (leg, name, k)
            assert np.isnan(out["angles"][miss]).all() and np.isnan(out["fk"][miss]).all()
            assert (out["status"][miss] == MISSING).all() and (out["nfev"][miss] == 0).all()
            assert np.array_equal(state, ref["angles"][-1]), (leg, name)


def test_arguments(hiplib):
    from seqikpy_amd.streaming import SeqikStream, solve_streamed, solve_streamed_in_time
    z = load_golden("df3d_100")
    pose, seg, b, seeds = leg_arrays(z, "RF")
    good = hiplib.leg_params_from_arrays(seg, b, seeds)
    lib = hiplib.load()
    handle = ctypes.c_void_p(1)
    lay = hiplib.planar_layout(8)
    legs = (hiplib.SeqikLegParams * 1)(good)
    rc = lib.seqik_stream_open_skip(ctypes.byref(handle), 1, legs, None, 4, 8, ctypes.byref(lay), 1, 2, 1, 0, None)
    assert rc == hiplib.ERR_ARG and not handle.value
    assert b"seqik_stream_open_skip" in lib.seqik_last_error() and b"dense layout" in lib.seqik_last_error()
    rc = lib.seqik_stream_open_skip(ctypes.byref(handle), 1, legs, None, 4, 8, None, 1, 0, 1, 0, None)
    assert rc == hiplib.ERR_ARG and b"bad sizes" in lib.seqik_last_error()
    assert lib.seqik_stream_get_carry(None, None, 1) == hiplib.ERR_ARG
    with pytest.raises(ValueError, match="missing key points"):
        SeqikStream([good], slab_seq=4, n_frames=8, missing="bogus")
    with pytest.raises(ValueError, match="dense layout"):
        SeqikStream([good], slab_seq=4, n_frames=8, layout=lay, missing="skip")
    with pytest.raises(ValueError, match="bad sizes"):
        SeqikStream([good], slab_seq=4, n_frames=8, n_slots=0, missing="skip")
    bad = pose[None, None, :8].copy()
    bad[0, 0, 3, 2, 1] = np.nan
    with pytest.raises(ValueError, match="Residuals are not finite"):
        solve_streamed(bad, [good], slab_seq=1)
    with pytest.raises(ValueError, match="Residuals are not finite"):
        solve_streamed_in_time(bad, [good], slab_frames=4)
    with pytest.raises(ValueError, match="missing key points"):
        solve_streamed(bad, [good], slab_seq=1, missing="fill")
    with pytest.raises(ValueError, match="missing key points"):
        solve_streamed_in_time(bad, [good], slab_frames=4, missing="fill")


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    if hiplib.load().seqik_device_count() < 1:
        pytest.fail("GPU tier needs a GPU: the HIP path must not be skipped silently")
    return hiplib


@pytest.fixture(scope="module")
def df3d():
    z = load_golden("df3d_100")
    legs = [str(l) for l in z["legs"]]
    return z, legs, np.stack([z[f"{l}_pose"] for l in legs])      # (6, 100, 5, 3)


@pytest.fixture(scope="module")
def sequences_case(lib, df3d):
    """Five jittered copies of df3d_100, one gap pattern per sequence, and the whole batch solved in skip mode."""
    z, legs, base = df3d
    rng = np.random.default_rng(50)
    S, (L, N) = 5, base.shape[:2]
    pose = np.stack([base + (1e-3 * rng.standard_normal(base.shape) if s else 0.0) for s in range(S)])
    miss = np.zeros((S, L, N), bool)
    miss[1, 2] = True                                 # one leg entirely missing
    miss[2, :, 0] = True                              # first frame
    miss[3, :, N - 1] = True                          # last frame
    miss[4] = rng.random((L, N)) < 0.3                # random 30 %, NaN and +-inf
    for s in range(S):
        for l in range(L):
            pose[s, l] = mark(pose[s, l], miss[s, l], rng, values=NON_FINITE)
    assert np.array_equal(np_missing(pose), miss)
    params = _params(lib, z, legs)
    return pose, miss, params, lib.solve_seq(pose, params, missing="skip")


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [1, 3])
def test_slabs_of_sequences_equal_one_skip_call(lib, sequences_case, n_slots):
    from seqikpy_amd.streaming import solve_streamed
    pose, miss, params, ref = sequences_case
    st = solve_streamed(pose, params, slab_seq=2, n_slots=n_slots, missing="skip")     # 2 + 2 + 1 sequences
    assert same(st["angles"], ref["angles"]) and same(st["fk"], ref["fk"])
    assert_nan_exactly_at(st, miss)
    no_fk = solve_streamed(pose, params, slab_seq=2, n_slots=n_slots, want_fk=False, missing="skip")
    assert no_fk["fk"] is None and same(no_fk["angles"], ref["angles"])


def _time_patterns(N, rng):
    """One pattern per leg of the carried run in slabs of 16 frames (six slabs and a 4-frame rest)."""
    return [frames(N), frames(N, (0, 23)), frames(N, (48, 64)), frames(N, 15, 31, 95), rng.random(N) < 0.3,
            frames(N, (0, N))]


@pytest.fixture(scope="module")
def time_case(lib, df3d):
    z, legs, base = df3d
    rng = np.random.default_rng(60)
    N = base.shape[1]
    miss = np.stack(_time_patterns(N, rng))
    pose = np.stack([mark(base[l], miss[l], rng, values=NON_FINITE) for l in range(len(legs))])[None]
    assert np.array_equal(np_missing(pose[0]), miss)
    params = _params(lib, z, legs)
    return pose, miss, params, lib.solve_seq(pose, params, missing="skip")


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [1, 3])
def test_carried_time_slabs_equal_the_unsplit_skip_solve(lib, time_case, n_slots):
    """The state must come from the last non-missing frame of a slab, not from its last slot, must survive a slab
    without a valid frame, and must be the seed state until a chain has seen one."""
    from seqikpy_amd.streaming import solve_streamed_in_time
    pose, miss, params, ref = time_case
    st = solve_streamed_in_time(pose, params, slab_frames=16, n_slots=n_slots, missing="skip")
    assert same(st["angles"], ref["angles"]) and same(st["fk"], ref["fk"])
    assert_nan_exactly_at(st, miss[None])
    no_fk = solve_streamed_in_time(pose, params, slab_frames=16, n_slots=n_slots, want_fk=False, missing="skip")
    assert no_fk["fk"] is None and same(no_fk["angles"], ref["angles"])


@pytest.mark.gpu
@pytest.mark.parametrize("frame_chunk", [0, 16])
def test_skip_stream_on_finite_input_equals_the_plain_stream(lib, df3d, frame_chunk):
    """Seed state == NULL on the device, chunk 0 of a chunked slab included."""
    from seqikpy_amd.streaming import solve_streamed_in_time
    z, legs, base = df3d
    params = _params(lib, z, legs)
    if frame_chunk:
        assert lib.frame_chunk_plan(48, frame_chunk)[2] > 1       # the slabs really are chunked
    plain = solve_streamed_in_time(base[None], params, slab_frames=48, frame_chunk=frame_chunk)
    skip = solve_streamed_in_time(base[None], params, slab_frames=48, frame_chunk=frame_chunk, missing="skip")
    assert np.isfinite(skip["angles"]).all()
    assert np.array_equal(skip["angles"], plain["angles"]) and np.array_equal(skip["fk"], plain["fk"])


@pytest.mark.gpu
def test_chunked_carried_skip_equals_the_direct_chunked_call_per_slab(lib):
    from seqikpy_amd.streaming import SeqikStream
    z = load_golden("df3d_1000")
    legs = [str(l) for l in z["legs"]]
    params = _params(lib, z, legs)
    base = np.stack([z[f"{l}_pose"][:300] for l in legs])
    rng = np.random.default_rng(70)
    N, T, fc = 300, 100, 16
    assert lib.frame_chunk_plan(T, fc)[2] > 1
    miss = np.stack([frames(N, (14, 19), (96, 105), 199, (200, 216)),       # chunk edge, slab edge, last frame, chunk 0
                     frames(N, (0, 40), (90, 100)) | (rng.random(N) < 0.1),
                     frames(N, (100, 200)),                                   # a whole slab
                     frames(N, (30, 34), 99, 100, (295, 300)),
                     rng.random(N) < 0.3,
                     frames(N)])
    pose = np.stack([mark(base[l], miss[l], rng, values=NON_FINITE) for l in range(6)])[None]
    state = lib.stream_seed_state(params)[None]
    with SeqikStream(params, 1, T, carry=True, frame_chunk=fc, missing="skip") as st:
        assert np.array_equal(st.get_carry(), state)
        for k in range(N // T):
            slab = np.ascontiguousarray(pose[:, :, k * T:(k + 1) * T])
            a, f = np.empty((1, 6, T, 7)), np.empty((1, 6, T, 9, 3))
            st.submit(slab, a, f)
            st.wait()
            ref = lib.solve_seq(slab, params, missing="skip", init_angles=state, frame_chunk=fc)
            assert ref["chunk_stats"]["chunks"] > 1
            assert same(a, ref["angles"]) and same(f, ref["fk"]), k
            assert_nan_exactly_at(dict(angles=a, fk=f), miss[None, :, k * T:(k + 1) * T], k)
            state = np_next_state_batch(a, state)
            assert np.array_equal(st.get_carry(), state), k


@pytest.mark.gpu
def test_generic_chain_carried_skip_stream(lib):
    from seqikpy_amd.streaming import SeqikStream
    zg = load_golden("generic_rf_100")
    legs = [str(l) for l in zg["legs"]]
    params = _params(lib, zg, legs)
    rng = np.random.default_rng(80)
    N, T = 100, 25
    miss = np.stack([frames(N, (0, 3), 24, (40, 52), 99) | (rng.random(N) < 0.1), frames(N, (25, 50), 74)])
    pose = np.stack([mark(zg[f"{l}_pose"], miss[i], rng, rows=(0, 4), values=NON_FINITE) for i, l in enumerate(legs)])[None]
    unread = int(np.flatnonzero(~miss[0])[10])
    pose[0, 0, unread, 2] = np.nan                    # row 2 is not read by the generic chain
    assert np.array_equal(np_missing(pose[0], "generic"), miss) and not miss[0, unread]
    ref = lib.solve_generic(pose, params, missing="skip")
    outs = []
    with SeqikStream(params, 1, T, carry=True, generic=True, n_slots=2, missing="skip") as st:
        assert np.array_equal(st.get_carry(), lib.stream_seed_state(params, generic=True)[None])
        for k in range(N // T):
            a, f = np.empty((1, 2, T, 7)), np.empty((1, 2, T, 9, 3))
            st.submit(np.ascontiguousarray(pose[:, :, k * T:(k + 1) * T]), a, f)
            outs.append((a, f))
        st.wait()
    got = dict(angles=np.concatenate([o[0] for o in outs], axis=2), fk=np.concatenate([o[1] for o in outs], axis=2))
    assert same(got["angles"], ref["angles"]) and same(got["fk"], ref["fk"])
    assert_nan_exactly_at(got, miss[None])


@pytest.mark.gpu
def test_fused_alignment_ignores_row_0(lib):
    from seqikpy_amd.streaming import solve_streamed, solve_streamed_in_time
    z = load_golden("df3d_1000")
    legs = ["RF", "LF"]
    params = _params(lib, z, legs)
    raw = np.stack([z[f"{l}_raw"][:100] for l in legs])
    aff = [lib.make_affine(raw[li, :, 0].mean(axis=0), 1.1, [0.1 * li, 0.2, -0.3]) for li in range(2)]
    rng = np.random.default_rng(90)
    N = 100
    miss = np.stack([frames(N, 15, (30, 50), 95), rng.random(N) < 0.2])
    gp = np.stack([mark(raw[l], miss[l], rng, rows=(1, 2, 3, 4), values=NON_FINITE) for l in range(2)])
    gp[0, 10, 0, 1] = np.nan                          # row 0 only: not read with the fused alignment
    gp[1, 20:25, 0, :] = np.inf
    assert not miss[0, 10]
    miss_aff = np_missing(gp, "seq", True)
    assert np.array_equal(miss_aff, miss) and not np.array_equal(np_missing(gp), miss)
    ref = lib.solve_seq(gp[None], params, affine=aff, missing="skip")
    st = solve_streamed_in_time(gp[None], params, slab_frames=16, affine=aff, missing="skip")
    assert same(st["angles"], ref["angles"]) and same(st["fk"], ref["fk"])
    assert_nan_exactly_at(st, miss[None])
    seqs = np.ascontiguousarray(gp.reshape(2, 4, 25, 5, 3).transpose(1, 0, 2, 3, 4))      # 4 sequences of 25 frames
    ref = lib.solve_seq(seqs, params, affine=aff, missing="skip")
    st = solve_streamed(seqs, params, slab_seq=3, affine=aff, missing="skip")
    assert same(st["angles"], ref["angles"]) and same(st["fk"], ref["fk"])


@pytest.mark.gpu
def test_carry_control(lib, time_case):
    from seqikpy_amd.streaming import SeqikStream
    pose, miss, params, ref = time_case
    T, n_slabs = 16, 6
    seed = lib.stream_seed_state(params)[None]

    def run(st):
        outs = []
        for k in range(n_slabs):
            a = np.empty((1, 6, T, 7))
            st.submit(np.ascontiguousarray(pose[:, :, k * T:(k + 1) * T]), a)
            outs.append(a)
        st.wait()
        return np.concatenate(outs, axis=2)

    with SeqikStream(params, 1, T, want_fk=False, n_slots=2, carry=True, missing="skip") as st:
        assert np.array_equal(st.get_carry(), seed)
        first = run(st)
        assert same(first, ref["angles"][:, :, :n_slabs * T])
        # the last non-missing angles per chain (frame 95 of leg 3 is missing); the seed state for the all-missing leg
        state = st.get_carry()
        assert np.array_equal(state, np_next_state_batch(ref["angles"][:, :, :n_slabs * T], seed))
        assert np.array_equal(state[0, 5], seed[0, 5]) and miss[5].all()
        assert np.array_equal(state[0, 3], ref["angles"][0, 3, 94]) and miss[3, 95]
        assert np.array_equal(st.get_carry(1), state)
        st.reset_carry()
        assert np.array_equal(st.get_carry(), seed)
        assert same(run(st), first)
        # set_carry, then one slab == the direct call from that state
        given = ref["angles"][:, :, 40].copy()
        assert np.isfinite(given[0, :5]).all()
        given[0, 5] = ref["angles"][0, 0, 41]
        st.set_carry(given)
        assert np.array_equal(st.get_carry(), given)
        slab = np.ascontiguousarray(pose[:, :, 64:64 + T])
        a = np.empty((1, 6, T, 7))
        st.submit(slab, a)
        st.wait()
        direct = lib.solve_seq(slab, params, missing="skip", init_angles=given, want_fk=False)
        assert same(a, direct["angles"])
        assert np.array_equal(st.get_carry(), np_next_state_batch(a, given))
    # a plain carried stream: no state before the first slab, then the last frame of the last slab
    finite = np.stack([load_golden("df3d_100")[f"{l}_pose"] for l in ("RF", "RM", "RH", "LF", "LM", "LH")])[None]
    with SeqikStream(params, 1, T, want_fk=False, n_slots=2, carry=True) as st:
        with pytest.raises(ValueError, match="no state yet"):
            st.get_carry()
        outs = []
        for k in range(2):
            a = np.empty((1, 6, T, 7))
            st.submit(np.ascontiguousarray(finite[:, :, k * T:(k + 1) * T]), a)
            outs.append(a)
        state = st.get_carry()
        st.wait()
        assert np.array_equal(state, outs[-1][:, :, -1])
        st.reset_carry()
        with pytest.raises(ValueError, match="no state yet"):
            st.get_carry()
    with SeqikStream(params, 1, T, want_fk=False, missing="skip") as st:
        with pytest.raises(ValueError, match="not opened with carry"):
            st.get_carry()
