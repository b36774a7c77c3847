"""Kernel trace of the skip-mode overhead at config-3 size (15625 x 6 x 64 frames, nothing missing, dense layout).

Three rounds of: a plain solve_seq_device, a second plain one straight after it, and compact -> solve_seq_device ->
expand (_lib.solve_seq_gaps_device), each followed by a synchronisation.  Run under
    rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python scripts/profile_gaps_skip.py
profiles/gaps_skip_kernel_trace_r08.csv is such a trace."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "sequential-inverse-kinematics_amd"))
import torch
from seqikpy_amd import _lib
from bench_support import make_workload
S, L, N = 15625, 6, 64
_, _, pose_np, params = make_workload(S, N, "iid", 7)
pose = torch.from_numpy(pose_np).cuda()
f = dict(dtype=torch.float64, device="cuda")
bufs = dict(d_angles=torch.empty((S, L, N, 7), **f), d_cpose=torch.empty_like(pose),
            d_map=torch.empty((S, L, N), dtype=torch.int32, device="cuda"),
            d_n_valid=torch.empty((S, L), dtype=torch.int32, device="cuda"),
            d_cangles=torch.empty((S, L, N, 7), **f), d_fk=torch.empty((S, L, N, 9, 3), **f),
            d_cfk=torch.empty((S, L, N, 9, 3), **f))
st = torch.cuda.current_stream().cuda_stream
for i in range(3):
    _lib.solve_seq_device(pose.data_ptr(), S, L, N, params, bufs["d_angles"].data_ptr(), bufs["d_fk"].data_ptr(), stream=st)
    torch.cuda.synchronize()
    _lib.solve_seq_device(bufs["d_cpose"].data_ptr() if i else pose.data_ptr(), S, L, N, params,
                          bufs["d_cangles"].data_ptr(), bufs["d_cfk"].data_ptr(), stream=st)
    torch.cuda.synchronize()
    _lib.solve_seq_gaps_device(pose, S, L, N, params, stream=st, **bufs)
    torch.cuda.synchronize()
print("done")
