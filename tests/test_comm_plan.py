"""CPU: the multi-GPU gather's rules over plain values (csrc/rt_comm_plan.{hpp,cpp}), driven through
the stand-alone tests/native/comm_plan_main.cpp -- built with plain g++ and once more with
-fsanitize=address,undefined (host code, no preload).  The expected answers are written out here from
the rules as rt_hip.h and the gather's design state them, never computed by the code under test:
* bands of 8 rows, band b to rank b % N, 16 bytes per pixel; adjacent bands merge into one run;
* a copy of `total` bytes is dealt over min(streams, total >> 20) transfer streams (at least 1; 1 with
  `split` off), each taking ceil(total / k) rounded up to 256 B, in image order;
* a plan is current for the same size and root with gathers left, and -- on the root of a copy-engine
  plan -- the same destination;
* a fresh plan links by address when every rank is in the call, by IPC handles with one rank per
  call in a world that can exchange them, and not at all for RCCL transfers."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mini-opencl-raytracer_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
MIB = 1 << 20


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def lines(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("comm_plan") / "comm_plan_main")
    flags = ["-O1", "-g"] + SANITIZE if request.param == "sanitized" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-o", exe, os.path.join(REPO, "tests", "native", "comm_plan_main.cpp"),
                    os.path.join(CSRC, "rt_comm_plan.cpp")], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return [ln.split() for ln in p.stdout.splitlines()]


def _parse_deal(words):
    """' runs a:b ... pieces s:r:at:n:d ...' -> (runs, pieces)"""
    i, j = words.index("runs"), words.index("pieces")
    runs = [tuple(map(int, w.split(":"))) for w in words[i + 1:j]]
    pieces = [tuple(map(int, w.split(":"))) for w in words[j + 1:]]
    return runs, pieces


def _band_runs(W, H, n, rank):
    """The rule, written out: band b (rows 8b .. 8b+7, the last one short) belongs to rank b % n."""
    runs = []
    for b in range((H + 7) // 8):
        if b % n != rank:
            continue
        off, size = b * 8 * W * 16, (min(8 * b + 8, H) - 8 * b) * W * 16
        if runs and runs[-1][0] + runs[-1][1] == off:
            runs[-1] = (runs[-1][0], runs[-1][1] + size)
        else:
            runs.append((off, size))
    return runs


def _check_deal(runs, pieces, streams, split):
    total = sum(n for _, n in runs)
    k = max(1, min(streams, total >> 20)) if split else 1
    share = (-(-total // k) + 255) // 256 * 256
    # the pieces tile every run exactly once, in image order; dense offsets are the running sum
    at_run, at_in_run, dense = 0, 0, 0
    carried = {}
    last_stream = 0
    for stream, run, at, n, d in pieces:
        assert n > 0 and run == at_run and at == at_in_run and d == dense, (runs, pieces)
        assert last_stream <= stream < k, (pieces, k)
        last_stream = stream
        carried[stream] = carried.get(stream, 0) + n
        if at != 0:  # a boundary inside a run
            assert dense % 256 == 0, (pieces, dense)
        dense += n
        at_in_run += n
        assert at_in_run <= runs[run][1]
        if at_in_run == runs[run][1]:
            at_run, at_in_run = at_run + 1, 0
    assert at_run == len(runs) and at_in_run == 0 and dense == total
    assert all(v <= share for v in carried.values()), (carried, share)
    if not split or total < 2 * MIB:
        assert [(s, r, a, n) for s, r, a, n, _ in pieces] == [(0, i, 0, n) for i, (_, n) in enumerate(runs)]
    else:  # every stream of the deal is used, the first ones to the full
        assert sorted(carried) == list(range(len(carried))) and len(carried) == -(-total // share)
        assert all(carried[s] == share for s in range(len(carried) - 1))


def test_deal_runs_sweep(lines):
    deals = [w for w in lines if w[0] == "deal"]
    seen = set()
    for w in deals:
        W, H, n, rank, streams, split = map(int, w[1:7])
        runs, pieces = _parse_deal(w)
        assert runs == _band_runs(W, H, n, rank), (W, H, n, rank)
        _check_deal(runs, pieces, streams, bool(split))
        seen.add((W, H, n, rank))
    # the sizes of the sweep, every rank of each; 5x7 at N = 4 has one band: ranks 1..3 have none
    want = {(3840, 2160, 1), (3840, 2160, 2), (3840, 2160, 8), (1277, 731, 3), (640, 37, 8), (5, 7, 4)}
    assert seen == {(W, H, n, r) for W, H, n in want for r in range(n)}
    assert len(deals) == len(seen) * 8 * 2
    assert _band_runs(5, 7, 4, 1) == [] and _band_runs(5, 7, 4, 0) == [(0, 560)]


def test_deal_runs_known_answers(lines):
    by = {tuple(w[1:7]): _parse_deal(w) for w in lines if w[0] == "deal"}
    # 3840x2160, one rank, 2 streams: one run of 132,710,400 B dealt as two pieces of 66,355,200 B
    runs, pieces = by[("3840", "2160", "1", "0", "2", "1")]
    assert runs == [(0, 132710400)]
    assert pieces == [(0, 0, 0, 66355200, 0), (1, 0, 66355200, 66355200, 66355200)]
    # ... and undivided with split off
    assert by[("3840", "2160", "1", "0", "2", "0")][1] == [(0, 0, 0, 132710400, 0)]
    # runs of 1, 2 and 1 MiB over 2 streams: shares of 2 MiB, the split inside the middle run
    (hand,) = [w for w in lines if w[:2] == ["hand", "three_runs"]]
    runs, pieces = _parse_deal(hand)
    assert runs == [(0, MIB), (4 * MIB, 2 * MIB), (16 * MIB, MIB)]
    assert pieces == [(0, 0, 0, MIB, 0), (0, 1, 0, MIB, MIB), (1, 1, MIB, MIB, 2 * MIB), (1, 2, 0, MIB, 3 * MIB)]


def test_plan_is_current(lines):
    got = {w[1]: int(w[2]) for w in lines if w[0] == "current"}
    assert got == {
        "same": 1, "width": 0, "height": 0, "root": 0,
        # the destination binds only the root of a copy-engine plan
        "not_root": 1, "not_ce": 1, "other_dst": 0, "other_dst_not_root": 1, "other_dst_not_ce": 1,
        # replan_after 10: gather 10 is the last of the plan
        "seq_before_end": 1, "seq_at_end": 0,
        "no_plan": 0,
    }


# rtp::Link and rtp::World in declaration order; RT_COMM_TRANSPORT_* from rt_hip.h
DIRECT, IPC, NONE, REFUSE = 0, 1, 2, 3
RANK, ALL, LOOPBACK, SHARED = 0, 1, 2, 3
COPY, RCCL, COPY_IPC = 0, 1, 2
# (transport, kind): n_local = 1 of 4, 4 of 4, 2 of 4, 1 of 1
LINKS = {
    (COPY, RANK): (IPC, DIRECT, NONE, DIRECT),
    (COPY, ALL): (IPC, DIRECT, NONE, DIRECT),
    (COPY, LOOPBACK): (NONE, DIRECT, NONE, DIRECT),  # (a loopback world has no way to pass handles around)
    (COPY, SHARED): (IPC, DIRECT, NONE, DIRECT),
    (RCCL, RANK): (NONE,) * 4, (RCCL, ALL): (NONE,) * 4, (RCCL, LOOPBACK): (NONE,) * 4, (RCCL, SHARED): (NONE,) * 4,
    # the IPC transport: one local communicator per call, never in a loopback world
    (COPY_IPC, RANK): (IPC, REFUSE, REFUSE, IPC),
    (COPY_IPC, ALL): (IPC, REFUSE, REFUSE, IPC),
    (COPY_IPC, LOOPBACK): (REFUSE,) * 4,
    (COPY_IPC, SHARED): (IPC, REFUSE, REFUSE, IPC),
}


def test_link_choice(lines):
    got = {(int(w[1]), int(w[2])): tuple(map(int, w[3:])) for w in lines if w[0] == "link"}
    assert got == LINKS


def test_enums_are_the_headers():
    import re
    with open(os.path.join(REPO, "include", "rt_hip.h")) as f:
        t = dict(re.findall(r"#define RT_COMM_TRANSPORT_(\w+) (\d+)", f.read()))
    assert (int(t["COPY_ENGINES"]), int(t["RCCL"]), int(t["COPY_ENGINES_IPC"])) == (COPY, RCCL, COPY_IPC)
    with open(os.path.join(CSRC, "rt_comm_plan.hpp")) as f:
        src = f.read()
    names = lambda enum: re.findall(r"^\s+(\w+),", re.search(r"enum class %s \{(.*?)\};" % enum, src, re.S).group(1), re.M)
    assert names("Link") == ["Direct", "Ipc", "None", "Refuse"]
    assert names("World") == ["RcclRank", "RcclAll", "Loopback", "Shared"]


def test_membership(lines):
    got = {w[1]: int(w[2]) for w in lines if w[0] == "members"}
    INVALID = -30  # RT_INVALID_VALUE
    assert got == {
        "all": 0, "one_missing": INVALID, "one_repeated": INVALID, "foreign_group": INVALID,
        "mixed_plain_first": INVALID, "mixed_loopback_first": INVALID, "no_loopback": 0,
        "world_of_64": 0, "rank_64": INVALID,
    }


def test_status_counts(lines):
    got = {w[1]: tuple(map(int, w[2:])) for w in lines if w[0] == "status"}
    # (active, bytes, copies) with runs of 100 + 50 bytes and a 4096-byte staging slot
    assert got == {
        "root_in_place": (COPY, 0, 0),
        "root_elsewhere": (COPY, 150, 2),      # its own bands straight into the destination
        "sender_direct": (COPY, 150, 4),       # pack + transfer per run
        "sender_ipc": (COPY_IPC, 150, 5),      # ... + the arrival flag
        "root_ipc_in_place": (COPY_IPC, 0, 0),
        "rccl": (RCCL, 4096, 1),
        "no_plan": (-1, 0, 0),
    }


def test_fold(lines):
    got = {w[1]: [float.fromhex(x) for x in w[2:]] for w in lines if w[0] == "fold"}
    eps = 2.0 ** -52
    # rank 0 first: (1 + 2^-53) + 2^-53 = 1 (each add rounds to even); (2^-53 + 2^-53) + 1 = 1 + 2^-52
    assert got["sum"] == [1.0, 1.0 + eps]
    assert got["max"] == [3.0, -0.5]
    assert got["in_place"] == [1.0, 1.0 + eps, 2.0 ** -53]


def test_units_are_pure():
    for name in ("rt_comm_plan.hpp", "rt_comm_plan.cpp", "rt_comm_files.hpp", "rt_comm_files.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            src = f.read()
        assert "#include <hip" not in src and "rccl" not in src, name
