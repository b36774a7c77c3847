"""The host-run rules of link frames, leg Jacobians, fit sensitivity and refinement (tests/harness/*.hip) against the
records the same harnesses produced at the commit before the units were moved onto one chain walk
(csrc/seqik_leg_chain.hpp): tests/golden/leg_records_pin.npz, written by tests/tools/leg_records_pin.py from a worktree of
that commit.  Bit for bit; CPU tier.  The GPU tier ties the kernels to these rules (test_link_frames.py, test_jacobians.py,
test_sensitivity.py, test_refine.py)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from harness_build import BUILD_DIR

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import leg_records_pin as pin  # noqa: E402

SENS_BAD_INPUT, REFINE_BAD_INPUT = 1 << 16, 1 << 24


@pytest.fixture(scope="module")
def pinned():
    return load_golden("leg_records_pin")


@pytest.fixture(scope="module")
def outputs(pinned):
    return pin.run_harnesses(os.path.join(ROOT, "tests", "harness"), BUILD_DIR, {k: pinned[k] for k in pin.INPUTS})


def test_the_fixture_holds_what_the_issue_lists(pinned):
    """The inputs are the ones tests/tools/leg_records_pin.py draws (so the fixture can be written again from the pinned
    commit), the hand-set rows are in them, and every output is finite in most rows and NaN (flags / info: the bad-input
    word) in the hand-set rows its unit reads: the pin cannot pass on an all-NaN record."""
    inp = pin.pin_inputs()
    for k in pin.INPUTS:
        assert pin.same_bits(np.asarray(inp[k], dtype=np.float64), pinned[k]), k
    assert pin.N == 32 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "leg_records_pin.npz")) < 200 * 1024
    lb, ub = pinned["bounds"][:, 0], pinned["bounds"][:, 1]
    for tag in ("seq", "gen"):
        a = pinned[f"angles_{tag}"]
        assert np.isnan(a[pin.ROW_NAN]).sum() == 1 and np.isinf(a[pin.ROW_INF]).sum() == 1
        assert (np.abs(a[pin.ROW_BEYOND]) > pin.ANGLE_MAX).sum() == 1 and np.isfinite(a[pin.ROW_BEYOND]).all()
        assert a[pin.ROW_UB, 6] == ub[6] and a[pin.ROW_LB, 1] == lb[1] and not a[pin.ROW_ZERO].any()
        ok = np.delete(a, pin.BAD_ANGLE_ROWS, axis=0)
        assert ((ok >= lb) & (ok <= ub)).all()
    assert (~np.isfinite(pinned["pose"])).sum() == 1 and not np.isfinite(pinned["pose"][pin.ROW_POSE]).all()
    assert (pinned["kp_weight"] == 0).sum() == 1 and pinned["kp_weight"][pin.ROW_WEIGHT, 1] == 0
    outs = [k for k in pinned.files if k not in pin.INPUTS]
    assert len(outs) == 4 + 6 + 3 + 3
    for k in outs:
        v = pinned[k]
        bad = pin.BAD_INPUT_ROWS if k.startswith(("sens", "std", "flags", "refine")) else pin.BAD_ANGLE_ROWS
        good = np.setdiff1d(np.arange(pin.N), bad)
        if v.dtype == np.int32:
            word = SENS_BAD_INPUT if k == "flags" else REFINE_BAD_INPUT
            assert (v[list(bad)] == word).all() and (v[good] != word).all() and (v[good] >= 0).all(), k
            continue
        v = v.reshape(pin.N, -1)
        if k == "sigma_gen":
            assert np.isnan(v[:, 3:]).all()   # the generic chain has three singular values
            v = v[:, :3]
        assert np.isnan(v[list(bad)]).all(), k
        # (a stage that is not positive definite makes part of a sensitivity row NaN by the rule: hence most, not all)
        assert np.isfinite(v[good]).all(axis=1).sum() >= (3 * len(good)) // 4, k


def test_the_rules_reproduce_the_pinned_records_bit_for_bit(pinned, outputs):
    """Every entry point of the four harnesses -- plain, staged, reduce-only -- on the pinned inputs == the pinned commit's
    record: uint64 view (int32 for flags and info)."""
    assert sorted({pin.stored_name(k) for k in outputs}) == sorted(k for k in pinned.files if k not in pin.INPUTS)
    assert len(outputs) == 2 * (4 + 6) + 4 + 3
    for name, got in outputs.items():
        want = pinned[pin.stored_name(name)]
        assert got.dtype == want.dtype and pin.same_bits(got, want), name
