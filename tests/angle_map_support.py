"""TEST INFRASTRUCTURE -- what the tests of the angle maps (forward kinematics, link frames, leg Jacobians) share: the
GPU-tier gate behind each file's `lib` fixture, leg parameters and stacked arrays from a golden fixture, the bit-for-bit
comparison, and a scope that sets the library's per-call environment switches."""
import contextlib
import os

import numpy as np
import pytest


def gpu_lib(hiplib):
    """The body of a `lib` fixture: the binding, or a failure where there is no GPU."""
    if hiplib.load().seqik_device_count() < 1:
        pytest.fail("GPU tier needs a GPU: the HIP path must not be skipped silently")
    return hiplib


def _params(lib, z, legs):
    return [lib.leg_params_from_arrays(z[f"{l}_seg"], z[f"{l}_bounds"], z[f"{l}_seeds"]) for l in legs]


def _generic_params(lib, z, legs):
    """The fixture's legs with mid-range seeds for the generic chain (seeded positionally in its own link order: roll,
    yaw, pitch, ...; the sequential seeds of the middle and hind legs lie outside those bounds)."""
    out = []
    for l in legs:
        seeds = z[f"{l}_seeds"].copy()
        seeds[19:26] = z[f"{l}_bounds"][[2, 0, 1, 3, 4, 5, 6]].mean(axis=1)
        out.append(lib.leg_params_from_arrays(z[f"{l}_seg"], z[f"{l}_bounds"], seeds))
    return out


def _stack(z, legs, key="pose", sl=slice(None)):
    return np.stack([z[f"{l}_{key}"][sl] for l in legs])[None]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


SENTINEL = -12345.678


def made_up_batch(S, L, N, seed):
    """(S, L, N, 7) angles in +-pi with a NaN and an out-of-domain record, L segment sets, (S, L, N, 3) origins."""
    rng = np.random.default_rng(seed)
    ang, org = rng.uniform(-np.pi, np.pi, (S, L, N, 7)), rng.standard_normal((S, L, N, 3))
    flat = ang.reshape(-1, 7)
    flat[len(flat) // 3, 4], flat[-1, 0] = np.nan, 1e300
    return ang, rng.uniform(0.15, 1.8, (L, 4)), org


def guarded(n, width):
    """A device buffer of n records of `width` doubles with one guard record on each side, all filled with a sentinel
    -> (the tensor, the address of record 0)."""
    import torch
    buf = torch.full(((n + 2) * width,), SENTINEL, dtype=torch.float64, device="cuda")
    return buf, buf.data_ptr() + 8 * width


def unguarded(buf, width):
    """The n records of a `guarded` buffer as numpy (n, width); asserts that both guards are untouched."""
    got = buf.cpu().numpy()
    assert (got[:width] == SENTINEL).all() and (got[-width:] == SENTINEL).all(), "guard record overwritten"
    return got[width:-width].reshape(-1, width)


@contextlib.contextmanager
def switches(**env):
    """The environment switches the library reads per call (SEQIK_FK_STAGED=..., ...), put back on the way out."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
