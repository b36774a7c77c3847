"""GPU tier: the device-side control path of a chunked call (seqik_chunk_verify / decide / scan kernels, the work-list
walks of seqik_chunk_kernel<REPAIR / SWEEP> and seqik_chunk_pipe_kernel<REPAIR / SERIAL>, launch_chunked) where MANY chunks
fail at once.  Yardstick: the batched replay model (tests/chunk_batch_model.py) whose every solve is the library's plain
serial call on the lane-per-chain kernel (pipeline=1, frame_chunk=0 -- pinned to the C oracle bit for bit by
tests/test_gpu_parity.py, and none of the chunk kernels), plus a seeded sample of chains replayed by ``ChunkedChain`` on
the C oracle itself.  Everything is compared by equality of bits and integers: angles, FK, chunk_states, chunk_flags and
the ten statistics.

Every case starts with "named-for" assertions, computed from the model and the restated launch arithmetic
(tests/chunk_model.py) alone: they FAIL when the input does not reach the branch the case is named for."""
import functools

import numpy as np
import pytest

from chunk_batch_model import Replay
from chunk_model import ChunkedChain, launch_shape, plan, repair_walk, serial_walk
from conftest import load_golden

pytestmark = pytest.mark.gpu
ORACLE_FRAMES_PER_CASE = 4000


class Ctx:
    def __init__(self, hiplib, oracle):
        from oracle import c_oracle
        from seqikpy_amd import data, utils
        self.lib, self.oracle, self.names = hiplib, oracle, list(data.LEGS)
        self.body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, self.names)
        self.params = [hiplib.make_leg_params(l, data.BOUNDS_LOCOMOTION, self.body, data.INITIAL_ANGLES_LOCOMOTION) for l in self.names]
        self.legs = [c_oracle.leg_params(l, data.BOUNDS_LOCOMOTION, self.body, data.INITIAL_ANGLES_LOCOMOTION) for l in self.names]
        self.models, self.samples = {}, {}

    def solve(self, pose, leg_index, init):
        """The model's solver: the plain serial call, one launch per leg of the batch."""
        ang, fk = np.empty(pose.shape[:2] + (7,)), np.empty(pose.shape[:2] + (9, 3))
        for l in np.unique(leg_index):
            sel = np.flatnonzero(leg_index == l)
            out = self.lib.solve_seq(pose[sel][:, None], [self.params[int(l)]], pipeline=1, frame_chunk=0,
                                     init_angles=None if init is None else init[sel][:, None])
            ang[sel], fk[sel] = out["angles"][:, 0], out["fk"][:, 0]
        return ang, fk

    @functools.lru_cache(maxsize=None)
    def iid(self, S, N):
        from seqikpy_amd import data, synthetic
        return synthetic.synthetic_pose(S, N, self.names, data.BOUNDS_LOCOMOTION, self.body, data.TEMPLATE_NMF_LOCOMOTION, variant="iid")

    def model(self, key, pose, chunk, halo, **kw):
        """The replay model of a call over pose (S, 6, N, 5, 3), computed once per `key` and left unchanged."""
        if key not in self.models:
            S, L, N = pose.shape[:3]
            self.models[key] = Replay(self.solve, pose.reshape(S * L, N, 5, 3), np.tile(np.arange(L), S), chunk, halo, **kw).run()
        return self.models[key]

    def oracle_sample(self, key, m, **kw):
        """6 to 8 chains of model `m`, picked by a seeded generator with a bias to chains with repairs, sweeps or the serial
        flag, replayed by ChunkedChain on the C oracle; as many of the 8 as ORACLE_FRAMES_PER_CASE leg-frames pay for, never
        fewer than 6.  Where six whole chains cost more than that (K = 100), each is replayed over its first chunks only,
        as many as the budget pays for: what happens to chunk k depends on the chunks up to k alone (without the guard, which
        counts over the whole chain).  -> [(chain, ChunkedChain)]"""
        if key not in self.samples:
            rng = np.random.default_rng(20240 + sum(map(ord, key)))
            w = 1.0 + 4.0 * ((m.chunk_flags & 2) != 0).any(1) + 4.0 * ((m.chunk_flags & 4) != 0).any(1) + 4.0 * m.serial
            if m.serial.any() and not m.serial.all():     # both paths in one call: half of the sample from either
                w[~m.serial] *= w[m.serial].sum() / w[~m.serial].sum()
            picks = list(rng.choice(m.n, size=min(8, m.n), replace=False, p=w / w.sum()))
            while len(picks) > 6 and m.solved_frames[picks].sum() > ORACLE_FRAMES_PER_CASE:
                picks.pop()
            cost, k_replayed = int(m.solved_frames[picks].sum()), m.K
            if cost > ORACLE_FRAMES_PER_CASE:
                assert not m.guard
                k_replayed = int(m.K * 0.95 * ORACLE_FRAMES_PER_CASE / cost)
            out, frames = [], 0
            for i in picks:
                c = ChunkedChain(self.oracle, m.pose[i, :m.span(k_replayed - 1)[1]], *self.legs[int(m.leg[i])], m.C, m.h, tol=m.tol,
                                 rounds=m.rounds, init=None if m.init is None else m.init[i].copy(), **kw)
                c.o = CountingOracle(self.oracle)
                c.speculate()
                c.settle()
                frames += c.o.frames
                out.append((int(i), c))
            assert frames <= ORACLE_FRAMES_PER_CASE, frames
            print(f"[chunk-control] oracle sample of {key}: chains {[i for i, _ in out]}, first {k_replayed} of {m.K} chunks, {frames} leg-frames")
            self.samples[key] = out
        return self.samples[key]


class CountingOracle:
    def __init__(self, oracle):
        self.oracle, self.frames = oracle, 0

    def seq_leg(self, pose, *a, **kw):
        self.frames += len(pose)
        return self.oracle.seq_leg(pose, *a, **kw)


@pytest.fixture(scope="module")
def ctx(hiplib, oracle):
    return Ctx(hiplib, oracle)


def run_device(ctx, d_pose, S, N, K, want_fk=True, planar=False, d_init=None, **opt):
    """One chunked call through the device entry point into zeroed buffers -> dict of tensors (dense shapes)."""
    import torch
    L = 6
    d_ang = torch.zeros((S, L, 7, N) if planar else (S, L, N, 7), dtype=torch.float64, device="cuda")
    d_fk = torch.zeros((S, L, N, 9, 3), dtype=torch.float64, device="cuda") if want_fk else None
    d_states = torch.zeros((S, L, K, 7), dtype=torch.float64, device="cuda")
    d_flags = torch.zeros((S, L, K), dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros(ctx.lib.N_CHUNK_STATS, dtype=torch.int32, device="cuda")
    ctx.lib.solve_seq_device(d_pose.data_ptr(), S, L, N, ctx.params, d_ang.data_ptr(), d_fk.data_ptr() if want_fk else 0,
                             layout=ctx.lib.planar_layout(N) if planar else None, d_init=d_init.data_ptr() if d_init is not None else 0,
                             d_chunk_stats=d_stats.data_ptr(), d_chunk_flags=d_flags.data_ptr(), d_chunk_states=d_states.data_ptr(), **opt)
    torch.cuda.synchronize()
    ctx.lib.check_faults()
    return dict(angles=d_ang.transpose(2, 3) if planar else d_ang, fk=d_fk, states=d_states, flags=d_flags, stats=d_stats)


def upload(pose, planar=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pose.transpose(0, 1, 3, 2, 4)) if planar else np.ascontiguousarray(pose)).cuda()


def assert_equals_model(out, m, sample, what):
    """Device result == model (every chain) == ChunkedChain on the oracle (the sampled chains), bits and integers."""
    lead = m.lead
    host = {k: (v.cpu().numpy().reshape((m.n,) + tuple(v.shape[2:])) if v is not None and k != "stats" else v) for k, v in out.items()}
    assert np.array_equal(host["angles"][:, lead:], m.angles[:, lead:]), what
    if host["fk"] is not None:
        assert np.array_equal(host["fk"][:, lead:], m.fk[:, lead:]), what
    assert np.array_equal(host["states"], m.chunk_states), what
    assert np.array_equal(host["flags"], m.chunk_flags), what
    got = out["stats"].cpu().numpy()[:10]
    assert np.array_equal(got, m.total_stats()), (what, got, m.total_stats())
    assert len(sample) >= min(6, m.n)
    for i, c in sample:                                   # (c may cover the first c.K chunks = c.N frames of the chain only)
        assert np.array_equal(host["angles"][i, lead:c.N], c.angles[lead:]), (what, i)
        if host["fk"] is not None:
            assert np.array_equal(host["fk"][i, lead:c.N], c.fk[lead:]), (what, i)
        assert np.array_equal(host["states"][i, :c.K], c.ss) and np.array_equal(host["flags"][i, :c.K], c.flags), (what, i)
        assert c.K < m.K or np.array_equal(m.stats[i], c.stats), (what, i)


def report(case, m, **more):
    print(f"[chunk-control] {case}: {m.counts()} {more}")


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [1, 2, 3])
@pytest.mark.parametrize("lanes", [1, 7, 64])
def test_straddle_first_check_counts_two_chains_in_one_wavefront(ctx, lanes, pipeline):
    """K = 12 is no divisor of 64: the wavefronts of the verify kernel straddle chain boundaries, and with iid poses several
    chains fail inside one of them (the second atomic, `else if (inc && c != c0)`)."""
    S, N, C, h = 4, 48, 4, 4
    pose = ctx.iid(S, N)
    m = ctx.model("straddle", pose, C, h)
    shape = launch_shape(S, 6, m.K, lanes, pipeline)
    walk = repair_walk(int(m.listed[0].sum()), shape)
    report("straddle", m, lanes=lanes, pipeline=pipeline, W=walk["W"])
    flat = np.zeros(-(-m.n * m.K // 64) * 64, bool)
    flat[:m.n * m.K] = m.failed_first.ravel()                       # thread t of the verify kernel: chain t / K, chunk t % K
    chain_of = np.minimum(np.arange(flat.size) // m.K, m.n - 1)
    chains_per_span = [len(set(chain_of[s:s + 64][flat[s:s + 64]])) for s in range(0, flat.size, 64)]
    assert m.K == 12 and max(chains_per_span) >= 2, chains_per_span
    assert shape["piped"] == (pipeline != 1)
    if lanes == 64:
        assert walk["W"] >= 2, walk
    out = run_device(ctx, upload(pose), S, N, m.K, frame_chunk=C, frame_halo=h, lanes_per_wave=lanes, pipeline=pipeline)
    assert_equals_model(out, m, ctx.oracle_sample("straddle", m), (lanes, pipeline))


THIN = dict(S=24, N=48, C=4, h=4)


def thin_model(ctx):
    pose = ctx.iid(THIN["S"], THIN["N"])
    m = ctx.model("thin", pose, THIN["C"], THIN["h"])
    return pose, m


@pytest.mark.parametrize("want_fk", [False, True])
@pytest.mark.parametrize("pipeline", [1, 2, 3])
def test_thin_waves_work_list_of_several_items_per_wave(ctx, pipeline, want_fk):
    """Full-width waves on a small call: the work list of a round is longer than the grid, so W = ceil(items / waves) > 1 and
    `cursor = wave * W + lane / lane_replication(W)`, with a replication that is neither 1 nor a multiple of 8 in round 1 and
    another W in a later round."""
    pose, m = thin_model(ctx)
    shape = launch_shape(THIN["S"], 6, m.K, 64, pipeline)
    walks = [repair_walk(int(r.sum()), shape) for r in m.listed]
    report("thin waves", m, pipeline=pipeline, fk=want_fk, W=[w["W"] for w in walks], waves=shape["repair_waves"])
    assert walks[0]["W"] >= 9 and walks[0]["replication"] not in (1, 8, 16, 32, 64) and walks[0]["replication"] % 8 != 0, walks
    assert any(2 <= w["W"] < walks[0]["W"] for w in walks[1:]), walks
    out = run_device(ctx, upload(pose), THIN["S"], THIN["N"], m.K, want_fk=want_fk, frame_chunk=THIN["C"], frame_halo=THIN["h"],
                     lanes_per_wave=64, pipeline=pipeline)
    assert_equals_model(out, m, ctx.oracle_sample("thin", m), (pipeline, want_fk))


@pytest.mark.parametrize("pipeline", [1, 2, 3])
def test_planar_layout_repairs_read_their_warm_start_with_the_joint_stride(ctx, pipeline):
    """The thin-waves call in the planar layout (angles [chain][7][frame]): a repair's warm start and the consistency check read
    the seven joints of a frame ang_dof = N elements apart."""
    pose, m = thin_model(ctx)
    layout = ctx.lib.planar_layout(THIN["N"])
    repairs = int(sum(r.sum() for r in m.listed) + m.swept.sum())
    report("planar", m, pipeline=pipeline, repairs=repairs, ang_dof=layout.ang_dof)
    assert repairs >= 100 and layout.ang_dof != 1 and layout.ang_dof == THIN["N"]
    out = run_device(ctx, upload(pose, planar=True), THIN["S"], THIN["N"], m.K, planar=True, frame_chunk=THIN["C"],
                     frame_halo=THIN["h"], lanes_per_wave=64, pipeline=pipeline)
    assert_equals_model(out, m, ctx.oracle_sample("thin", m), pipeline)


@pytest.mark.parametrize("pipeline", [1, 2])
def test_long_sweep_goes_past_its_first_64_chunks(ctx, pipeline):
    """K = 100 with a run-in of one frame and one repair round: the sweep starts with inconsistent chunks behind chunk 64 (the
    wave's cursor gets there one re-solved chunk at a time: every span of 64 it verifies holds an inconsistent chunk)."""
    S, N, C, h = 2, 400, 4, 1
    pose = ctx.iid(S, N)
    m = ctx.model("sweep", pose, C, h, rounds=1)
    report("long sweep", m, pipeline=pipeline, chains_pending_behind_64=int(m.pending_at_sweep[:, 64:].any(1).sum()))
    assert m.K == 100 and m.pending_at_sweep[:, 64:].any() and m.swept[:, 64:].any()
    out = run_device(ctx, upload(pose), S, N, m.K, frame_chunk=C, frame_halo=h, chunk_rounds=1, pipeline=pipeline)
    assert_equals_model(out, m, ctx.oracle_sample("sweep", m), pipeline)


def test_long_sweep_skips_a_span_of_64_consistent_chunks(ctx):
    """A quiet head: 264 recorded frames (66 chunks that pass) in front of 36 frames of iid poses.  The sweep's first span of 64
    chunks holds nothing to do, `cursor += 64` runs, and the work is all behind it."""
    S, N, C, h = 2, 300, 4, 4
    z = load_golden("df3d_1000")
    pose = ctx.iid(S, N).copy()
    for s, at in ((0, 0), (1, 500)):
        pose[s, :, :264] = np.stack([z[f"{l}_pose"][at:at + 264] for l in ctx.names])
    m = ctx.model("sweep-quiet-head", pose, C, h, rounds=1)
    quiet = ~m.pending_at_sweep[:, :m.k_first + 64].any(1) & m.pending_at_sweep.any(1)
    report("long sweep, quiet head", m, chains_with_a_quiet_first_span=int(quiet.sum()))
    assert m.K == 75 and quiet.sum() >= 2
    out = run_device(ctx, upload(pose), S, N, m.K, frame_chunk=C, frame_halo=h, chunk_rounds=1)
    assert_equals_model(out, m, ctx.oracle_sample("sweep-quiet-head", m), "quiet head")


def test_exact_tolerance_is_the_serial_walk(ctx):
    """chunk_tol < 0: a chunk is kept only if its run-in reproduced the true state bit for bit; one chunk per chain is listed per
    round, the sweep does the rest -> the serial walk, bit for bit."""
    S, N, C, h = 3, 96, 8, 2
    pose = ctx.iid(S, N)
    m = ctx.model("exact", pose, C, h, tol=0.0, rounds=2)
    report("exact", m)
    serial_ang, serial_fk = ctx.solve(m.pose, m.leg, None)
    assert np.array_equal(m.angles, serial_ang) and np.array_equal(m.fk, serial_fk)
    assert m.failed_first.sum() > m.n * (m.K - 1) // 2 and m.swept.sum() > 2 * m.n
    out = run_device(ctx, upload(pose), S, N, m.K, frame_chunk=C, frame_halo=h, chunk_tol=-1.0, chunk_rounds=2)
    assert np.array_equal(out["angles"].cpu().numpy().reshape(m.n, N, 7), serial_ang)
    assert np.array_equal(out["fk"].cpu().numpy().reshape(m.n, N, 9, 3), serial_fk)
    assert int(out["stats"][6]) == int(m.swept.sum())
    assert_equals_model(out, m, ctx.oracle_sample("exact", m), "exact")


@pytest.mark.parametrize("pipeline", [1, 2])
def test_lead_and_init_chunk_zero_on_the_work_list_beside_other_chunks(ctx, pipeline):
    """A slab with a run-in in front of chunk 0 and the caller's state in front of it: the true one for the even chains, 1e-3 rad
    off for the odd ones, whose chunk 0 (k_first = 0) is listed in round 1 together with the other failing chunks."""
    import torch
    S, C, h, lead = 8, 8, 8, 8
    N = lead + 96
    pose = ctx.iid(S, N)
    flat = pose.reshape(S * 6, N, 5, 3)
    leg = np.tile(np.arange(6), S)
    if "lead-init" not in ctx.models:
        ctx.true_state = ctx.solve(flat[:, :lead], leg, None)[0][:, -1]      # what the run-in of chunk 0 arrives at
    odd = np.arange(S * 6) % 2 == 1
    ub = np.stack([ctx.legs[l][1][:, 1] for l in leg])
    off = np.where(ctx.true_state + 1e-3 <= ub, 1e-3, -1e-3)                # a joint that sits on its upper limit: 1e-3 rad the other way
    init = ctx.true_state + off * odd[:, None]                               # (a warm start outside the limits is no valid input)
    assert np.all(init >= np.stack([ctx.legs[l][1][:, 0] for l in leg])) and np.all(init <= ub)
    m = ctx.model("lead-init", pose, C, h, init=init, lead=lead)
    report("lead + init", m, pipeline=pipeline, chunk0_listed=int(m.listed[0][:, 0].sum()))
    assert m.k_first == 0 and m.K == 12
    assert np.array_equal(m.listed[0][:, 0], odd) and np.array_equal(m.failed_first[:, 0], odd)
    assert m.listed[0][:, 1:].sum() > 0 and m.listed[0][~odd, 1:].sum() > 0
    out = run_device(ctx, upload(pose), S, N, m.K, d_init=torch.from_numpy(init.reshape(S, 6, 7)).cuda(), frame_chunk=C, frame_halo=h,
                     frame_lead=lead, pipeline=pipeline)
    assert_equals_model(out, m, ctx.oracle_sample("lead-init", m, lead=lead), pipeline)


def serial_batch(ctx):
    """250 sequences of 48 frames in the automatic mode: iid poses send almost every chain to the serial walk; the last two
    sequences are windows of a recording, whose chains keep their chunks -- both paths in one call."""
    S, N = 250, 48
    z = load_golden("df3d_1000")
    pose = ctx.iid(S, N).copy()
    for s, at in ((S - 2, 100), (S - 1, 640)):
        pose[s] = np.stack([z[f"{l}_pose"][at:at + N] for l in ctx.names])
    C, h, K = plan(N)
    m = ctx.model("serial", pose, C, h, guard=True)
    return pose, m


def test_serial_walk_of_more_chains_than_workgroups(ctx):
    pose, m = serial_batch(ctx)
    S, N = pose.shape[0], pose.shape[2]
    walk = serial_walk(int(m.serial.sum()), m.n)
    report("serial, paired", m, walk=walk)
    assert (m.C, m.h, m.K) == (4, 4, 12)
    assert m.serial.sum() > 1024 and walk["W"] == 2 and not walk["roomy"]
    assert (~m.serial).sum() >= 1 and not m.serial[-12:].any()
    out = run_device(ctx, upload(pose), S, N, m.K, frame_chunk=-1)
    assert_equals_model(out, m, ctx.oracle_sample("serial", m, guard=True), "serial")


def tiled_call(ctx, pose, m, n_seq, **opt):
    """The base call `pose` (S0 sequences) tiled on the device to n_seq sequences (whole tiles and a leading part of one),
    compared tile by tile on the device with the base's expected arrays; statistics = the sum over the chains of the call."""
    import torch
    S0, N = pose.shape[0], pose.shape[2]
    tiles = -(-n_seq // S0)
    d_pose = upload(pose).repeat(tiles, 1, 1, 1, 1)[:n_seq].contiguous()
    out = run_device(ctx, d_pose, n_seq, N, m.K, want_fk=False, **opt)
    del d_pose
    want = dict(angles=torch.from_numpy(m.angles.reshape(S0, 6, N, 7)).cuda(), states=torch.from_numpy(m.chunk_states.reshape(S0, 6, m.K, 7)).cuda(),
                flags=torch.from_numpy(m.chunk_flags.reshape(S0, 6, m.K)).cuda())
    for t in range(tiles):
        n = min(S0, n_seq - t * S0)
        for k, w in want.items():
            assert torch.equal(out[k][t * S0:t * S0 + n], w[:n]), (k, t)
    per_seq = m.stats.reshape(S0, 6, 16).sum(1).astype(np.int64)
    stats = (n_seq // S0) * per_seq.sum(0) + per_seq[:n_seq % S0].sum(0)
    stats[1:3] = (m.C, m.h)
    got = out["stats"].cpu().numpy()
    assert np.array_equal(got[:10], stats[:10]), (got, stats)


def base_equals_oracle_sample(m, sample):
    """The expected arrays of a tiled case (the model of the base call) against ChunkedChain on the oracle itself."""
    assert len(sample) >= 6
    for i, c in sample:
        assert np.array_equal(m.angles[i, :c.N], c.angles) and np.array_equal(m.chunk_states[i, :c.K], c.ss), i
        assert np.array_equal(m.chunk_flags[i, :c.K], c.flags), i


def test_capped_work_list_lanes_take_a_second_entry(ctx):
    """Under the 1024-workgroup cap of the pipeline's REPAIR kernel: W = 20, W = 40, and W = 64 with a second pass, in which a lane
    takes a second work-list entry and its ring counters carry over (`base` of pipe_run); the last size once more on the
    lane-per-chunk kernel under its 4096-wave cap.  A chain's result does not depend on what else is in the call, so every tile
    must equal the base call, which the model solves once."""
    S0, N, C, h = 64, 192, 4, 4
    pose = ctx.iid(S0, N)
    m = ctx.model("worklist", pose, C, h)
    listed_per_seq = np.cumsum(m.listed[0].reshape(S0, -1).sum(1))

    def listed(n_seq):
        return int((n_seq // S0) * listed_per_seq[-1] + (listed_per_seq[n_seq % S0 - 1] if n_seq % S0 else 0))

    def walk(n_seq, pipeline):
        return repair_walk(listed(n_seq), launch_shape(n_seq, 6, m.K, 0, pipeline))

    def sequences_for(target_w=None, second_pass=False):      # the smallest call that reaches it: whole tiles if any does
        sizes = [f * S0 for f in range(1, 64)] + list(range(S0, 64 * S0))
        return next(n for n in sizes if (walk(n, 2)["passes"] >= 2 if second_pass else walk(n, 2)["W"] == target_w))
    sizes = [sequences_for(20), sequences_for(40), sequences_for(second_pass=True)]
    report("capped work list", m, sequences=sizes, listed_round_1=[listed(n) for n in sizes], walks=[walk(n, 2) for n in sizes],
           lane_per_chunk=walk(sizes[2], 1))
    assert [walk(n, 2)["W"] for n in sizes] == [20, 40, 64] and walk(sizes[2], 2)["passes"] == 2 and listed(sizes[2]) > 65536
    assert launch_shape(sizes[2], 6, m.K, 0, 1)["repair_waves"] == 4096 and walk(sizes[2], 1)["W"] >= 2
    base_equals_oracle_sample(m, ctx.oracle_sample("worklist", m))
    for n_seq in sizes:
        tiled_call(ctx, pose, m, n_seq, frame_chunk=C, frame_halo=h, pipeline=2)
    tiled_call(ctx, pose, m, sizes[2], frame_chunk=C, frame_halo=h, pipeline=1)


def test_capped_serial_list_workgroups_take_a_second_chain(ctx):
    """More than 65 536 chains on the serial list: under the 1024-workgroup cap at W = 64 a lane of the SERIAL walk takes a second
    chain (`base` carried from one chain to the next)."""
    pose, m = serial_batch(ctx)
    S0 = pose.shape[0]
    n_serial = int(m.serial.sum())
    tiles = 65536 // n_serial + 1
    walk = serial_walk(tiles * n_serial, tiles * m.n)
    report("capped serial list", m, tiles=tiles, serial=tiles * n_serial, walk=walk)
    assert tiles * n_serial > 65536 and walk == dict(W=64, passes=2, roomy=False)
    base_equals_oracle_sample(m, ctx.oracle_sample("serial", m, guard=True))
    tiled_call(ctx, pose, m, tiles * S0, frame_chunk=-1)
