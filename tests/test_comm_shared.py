"""GPU: a world of separate processes on the one GPU of the test box (rtCommInitShared: setup
through files, no RCCL, which refuses two ranks on one device).  The gathers then take the path
the one-process-per-GPU setup takes between GPUs -- IPC handles of the root's receive slots and
flags exchanged and mapped, the link handshake, copy-engine copies into another process's memory,
arrival and slot-free flags written into another process's memory and waited on -- over several
pipelined steps (slots reused); only the copy between two GPUs over xGMI is not exercised.  The
gathered image must be byte-identical to an unsharded render."""
import os
import subprocess
import sys

import numpy as np
import pytest

from clrt import _native as N
from hip_helpers import HipRenderer

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("n,root,W,H", [(2, 0, 640, 360), (3, 1, 517, 203)])
def test_shared_world_gather_equals_unsharded(cornell, tmp_path, n, root, W, H):
    steps = 4
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "shared_worker.py"), str(tmp_path), str(n),
                               str(q), str(W), str(H), str(steps), str(root)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for q in range(n)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=100)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-1500:] for o in outs)
    got = np.load(tmp_path / "gathered.npy")
    r = HipRenderer(cornell, W, H, math=N.MATH_SHIPPED)
    for step in range(steps):
        r.frame(1 + 8 * step, n_frames=8)
    want = r.result()
    r.close()
    assert got.tobytes() == want.tobytes(), f"{(got != want).any(axis=1).sum()} pixels differ"


def test_shared_world_refuses_rccl_and_bad_arguments(tmp_path):
    import clrt
    from clrt import multigpu as mg
    ctx = clrt.CLContext(0)
    with pytest.raises(Exception):
        mg.Comm.init_shared(ctx, 2, 2, str(tmp_path))
    comm = mg.Comm.init_shared(ctx, 1, 0, str(tmp_path))
    with pytest.raises(Exception):
        comm.set_transport(N.COMM_TRANSPORT_RCCL)
    comm.set_transport(N.COMM_TRANSPORT_COPY_ENGINES)
    mg.Comm.barrier([comm])
    comm.destroy()
    # the directory now holds that world's id: a new world there is refused (its exchange files
    # could be read as the new world's)
    with pytest.raises(Exception) as e:
        mg.Comm.init_shared(ctx, 1, 0, str(tmp_path))
    assert e.value.code == -30
    ctx.release()


def test_failed_link_leaves_no_plan(cornell, tmp_path):
    """A plan is committed only when it is built and linked.  A shared world of one rank whose link
    step is refused (the test hook: a status code, nothing faults) has no RCCL to fall back to, so
    the gather fails -- and leaves no plan: no active transport, no pin on the destination.  The next
    gather plans and links afresh and moves the rendered bytes."""
    from clrt import multigpu as mg
    W, H = 64, 40
    r = HipRenderer(cornell, W, H, math=N.MATH_SHIPPED)
    comm = mg.Comm.init_shared(r.ctx, 1, 0, str(tmp_path))
    comm.set_transport(N.COMM_TRANSPORT_COPY_ENGINES_IPC)
    comm.shard(r.k)
    dst = r.ctx.create_buffer(N.MEM_READ_WRITE, W * H * 16)
    r.frame(1, n_frames=2)
    comm.set_option(N.COMM_OPT_FAIL_LINKS, 1)
    with pytest.raises(N.RTError) as e:
        mg.Comm.gather_bands([comm], [r.out], W, H, root=0, dst=dst)
    assert e.value.code == -59  # RT_INVALID_OPERATION
    assert comm.transport() == (N.COMM_TRANSPORT_COPY_ENGINES_IPC, -1)
    comm.set_option(N.COMM_OPT_FAIL_LINKS, 0)
    mg.Comm.gather_bands([comm], [r.out], W, H, root=0, dst=dst)
    assert comm.transport() == (N.COMM_TRANSPORT_COPY_ENGINES_IPC, N.COMM_TRANSPORT_COPY_ENGINES_IPC)
    got = np.zeros((W * H, 4), np.float32)
    r.ctx.ReadBuffer(dst, got, blocking=True)
    assert got.tobytes() == r.result().tobytes()
    comm.destroy()
    assert N.hip_lib().rtReleaseBuffer(dst.handle) == 0  # (no pin is left: freed here)
    dst.handle = None
    r.close()
