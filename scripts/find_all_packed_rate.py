#!/usr/bin/env python3
"""Every match of every packed row: the packed find-all entries against converting the batch first.  The rows are bench.py's c2r / c3r
rows (make_pattern / make_rows, per-row lengths (r * 2654435761) % 256 + 1), packed back to back on the device; c2p `[0-9]+` takes the RUN
transducer, c3p (the 1000-keyword dictionary) the lengths transducer.  Routes, timed by HIP events in one process, ALTERNATING (one step
of each route per round, W warm-up rounds, then K rounds):
  (a)  needle_find_all_compact16_packed_dev                     one walk of the packed text (more = NULL: no synchronisation)
  (a') needle_count_matches_packed_dev + torch cumsum + needle_find_all_csr_packed_dev
  (b)  needle_rows_from_packed_dev (stride 256) + needle_find_all_compact16_dev on its output
  (b') the same conversion + needle_count_matches_dev + cumsum + needle_find_all_csr_dev
  (c)  needle_find_all_compact16_dev on the fixed-stride ragged 256-byte rows
Per route: matches, a start / end checksum (all must agree), the median ms per step (min / max besides), GB/s over ACTUAL bytes -- chars + 8 B offset per row + result
bytes (compact16: offsets + 4 B per match; CSR: 4 B count per row + offsets + 8 B per match) -- and that rate's share of 8 TB/s.
The compact16 routes' scratch (n_rows / 64 x max_per_row x 256 B: 5 GB here) is above the library's default scratch keep (512 MB): this
script raises NEEDLE_SCRATCH_KEEP_MB (unless set) so that no timed step pays a fresh driver allocation.
Patterns WITHOUT a transducer (--only c3np,c2n): count + CSR fill through the packed entries on (a) the per-lane kernel
(needle_packed_find_all_lane.h) and (b) the conversion route (NEEDLE_PACKED_FIND_ALL_LANE=0).  The switch is read once per process, so
every route runs in a child of its own, alternating (a, b, a, b), one GPU process at a time, each under its own time limit; totals
and start / end checksums must agree.
  c3np  c3p's text, the dictionary extended by w[:3] and w[3:-1] of the first 100 keywords of at least --nested-min-len chars, longest
        first (a nested dictionary: no transducer -- asserted)
  c2n   c2p's text, the nullable `[0-9]*`
Big dictionaries (--only c3sp,c3xp,longp): count + CSR fill through the packed entries on (a) the n-gram filter kernel's find-all form
(needle_ngram_packed.h) and (b) the conversion route (NEEDLE_FIND_ALL_FILTER_PACKED=0: the route of the commit before the filter route),
children alternating as above; every child also reports the filter launches (forwards) of its timed steps.
  c3sp  bench.py's c3s rows (1000 keywords of 6 .. 8 chars: the compressed automaton), lengths uniform in [1, 256], packed
  c3xp  c3x (3000 keywords: walks out of HBM / L2), the same
  longp c3s's dictionary over 2000 short rows, one row of 70 000 and one of 200 000 chars (a keyword every ~1400 chars); --rows is ignored
python scripts/find_all_packed_rate.py [--rows N] [--steps K] [--warmup W] [--only c2p,c3p,c3np,c2n,c3sp,c3xp,longp] [--max-per-row M]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
os.environ.setdefault("NEEDLE_SCRATCH_KEEP_MB", "16384")


LANE_WORKLOADS = ("c3np", "c2n")
FILTER_WORKLOADS = ("c3sp", "c3xp", "longp")
# workload -> (the route's switch, what find_all_packed_route / find_all_packed_filter say with the switch on)
SWITCH = {wl: ("NEEDLE_PACKED_FIND_ALL_LANE", "lane") for wl in LANE_WORKLOADS}
SWITCH.update({wl: ("NEEDLE_FIND_ALL_FILTER_PACKED", "filter") for wl in FILTER_WORKLOADS})


def long_rows_batch(words, dev):
    """(data, offsets) of the long-row batch: 2000 short rows of c3s's text, a row of 70 000 and one of 200 000 chars among them."""
    import numpy as np
    import torch
    from needle_amd import workload as W
    rng = np.random.default_rng(17)
    host = W.keyword_batch(np, words, 0, 2000, 256)
    lens = np.arange(2000) * 2654435761 % 256 + 1
    rows = [host[i, :lens[i]] for i in range(2000)]
    al = np.array([ord(c) for c in "abcdefghijklmnopqrstuvwxyz "], dtype=np.uint8)
    for at, n in ((777, 70000), (1411, 200000)):
        r = rng.choice(al, n).astype(np.uint8)
        for k in range(n // 1400):
            w = np.array([ord(c) for c in words[k % len(words)]], dtype=np.uint8)
            r[100 + 1400 * k:100 + 1400 * k + w.size] = w
        rows.insert(at, r)
    text = np.concatenate(rows)
    text = np.concatenate([text, np.zeros((-text.size) % 4, np.uint8)])
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([r.size for r in rows])
    return torch.from_numpy(text).to(dev), torch.from_numpy(offsets).to(dev)


def lane_pattern(wl, nested_min_len):
    """(pattern, label, the base workload whose rows it scans, its planted words)"""
    import bench
    from needle_amd.pattern import DFACompiler
    if wl in FILTER_WORKLOADS:
        base = "c3x" if wl == "c3xp" else "c3s"
        pattern, what, words = bench.make_pattern(base)
        return pattern, what + (" -- the long-row batch" if wl == "longp" else ", per-row lengths uniform in [1, 256], packed"), base, words
    if wl == "c2n":
        _, _, words = bench.make_pattern("c2")
        return DFACompiler.compile("[0-9]*", "DigitStar"), "'[0-9]*' (nullable) over c2p's text", "c2", words
    _, _, words = bench.make_pattern("c3")
    long = [w for w in words if len(w) >= nested_min_len][:100]
    ext = sorted(set(words) | {w[:3] for w in long} | {w[3:-1] for w in long if w[3:-1]}, key=lambda w: (-len(w), w))
    return (DFACompiler.compile("|".join(ext), "Keywords1kNested"),
            "union-of-1k-keywords + %d prefixes / middles of %d keywords of >= %d chars (nested) over c3p's text" % (len(ext) - len(set(words)), len(long), nested_min_len),
            "c3", words)


def lane_child(args, wl):
    """One workload on the route this process's environment selects: count + cumsum + CSR fill, timed by events."""
    import torch
    import bench
    from needle_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = args.rows
    pattern, what, base, words = lane_pattern(wl, args.nested_min_len)
    assert pattern.find_all_transducer(1) is None, "%s: the pattern has a transducer" % wl
    route = pattern.find_all_packed_route(1, False)
    assert route == pattern.find_all_packed_route(1, True)
    if route == "conversion" and pattern.find_all_packed_filter(1, False):
        assert pattern.find_all_packed_filter(1, True)
        route = "filter"
    stream = torch.cuda.current_stream(dev).cuda_stream
    if wl == "longp":
        data, offsets = long_rows_batch(words, dev)
        n = offsets.numel() - 1
        chars = int(offsets[-1].item())
    else:
        lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(lens, 0)
        col = torch.arange(256, device=dev)[None, :]
        chars = int(offsets[-1].item())
        rows = bench.make_rows(base, words, 0, n, dev)
        data = torch.empty(chars, dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 20):
            k = min(1 << 20, n - s)
            data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
        del rows
    pv = _lib.PackedView()
    pv.data, pv.char_width, pv.n_rows, pv.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
    h = pattern._h

    def check(rc):
        assert rc == 0, L.needle_last_error()

    counts = torch.empty(n, dtype=torch.int32, device=dev)
    check(L.needle_count_matches_packed_dev(h, ctypes.byref(pv), counts.data_ptr(), stream))
    m = int(counts.to(torch.int64).sum().item())
    csr_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    st = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
    en = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)

    def step():
        check(L.needle_count_matches_packed_dev(h, ctypes.byref(pv), counts.data_ptr(), stream))
        torch.cumsum(counts, 0, out=csr_off[1:])
        check(L.needle_find_all_csr_packed_dev(h, ctypes.byref(pv), csr_off.data_ptr(), st.data_ptr(), en.data_ptr(), None, stream))

    step()
    torch.cuda.synchronize()
    assert int(csr_off[-1].item()) == m
    sums = (m, int(st.to(torch.int64).sum().item()), int(en.to(torch.int64).sum().item()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    launches = 0
    for r in range(args.warmup + args.steps):
        if r == args.warmup:
            launches = pattern.prefilter_state("forwards")["filter_launches"]
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        if r >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    launches = pattern.prefilter_state("forwards")["filter_launches"] - launches
    actual = chars + n * 8 + (n * 8 + 8) + n * 4 + m * 8
    med = sorted(ms)[len(ms) // 2]
    print(json.dumps({"workload": wl, "what": what, "route": route, "rows": n, "chars": chars, "matches": sums[0], "checksum_start": sums[1],
                      "checksum_end": sums[2], "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "GB/s": round(actual / med / 1e6, 1), "actual_bytes": actual, "filter_launches_per_step": round(launches / max(len(ms), 1), 2)}), flush=True)


def lane_parent(args, wl):
    """(a) the lane / filter route, (b) conversion, (a), (b): one child at a time.  This process never opens the GPU."""
    import subprocess
    runs = []
    switch, name = SWITCH[wl]
    for tag, env_val in (("a", "1"), ("b", "0"), ("a", "1"), ("b", "0")):
        env = dict(os.environ, **{switch: env_val})
        cmd = [sys.executable, os.path.abspath(__file__), "--lane-child", wl, "--rows", str(args.rows), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--nested-min-len", str(args.nested_min_len)]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=args.child_timeout, check=True)
        out = json.loads(r.stdout.decode().strip().split("\n")[-1])
        assert out["route"] == (name if tag == "a" else "conversion"), out
        out["tag"] = tag
        runs.append(out)
        print(json.dumps(out), flush=True)
    same = {(r["matches"], r["checksum_start"], r["checksum_end"]) for r in runs}
    assert len(same) == 1, same  # every route and run: the same matches
    a = [r["ms"] for r in runs if r["tag"] == "a"]
    b = [r["ms"] for r in runs if r["tag"] == "b"]
    print(json.dumps({"workload": wl, "summary": True, "matches": runs[0]["matches"], name + "_ms": a, "conversion_ms": b,
                      name + "_over_conversion": round((sum(a) / len(a)) / (sum(b) / len(b)), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lane-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--nested-min-len", type=int, default=5)  # (c3's keywords have 3..5 chars: its longest)
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="c2p,c3p")
    ap.add_argument("--max-per-row", type=int, default=128)
    args = ap.parse_args()
    if args.lane_child:
        return lane_child(args, args.lane_child)
    wanted = args.only.split(",")
    for wl in wanted:
        if wl in SWITCH:
            lane_parent(args, wl)
    args.only = ",".join(w for w in wanted if w not in SWITCH)
    if not args.only:
        return
    import torch
    import bench
    from needle_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = args.rows
    mpr = args.max_per_row
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    l32 = lens.to(torch.int32)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    chars = int(offsets[-1].item())
    stream = torch.cuda.current_stream(dev).cuda_stream

    def check(rc):
        assert rc == 0, L.needle_last_error()

    for wl in args.only.split(","):
        base = {"c2p": "c2", "c3p": "c3"}[wl]
        pattern, what, words = bench.make_pattern(base)
        h = pattern._h
        kind = pattern.find_all_transducer(1)["kind"]
        rows = bench.make_rows(base, words, 0, n, dev)
        data = torch.empty(chars, dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 20):  # packed slab by slab
            k = min(1 << 20, n - s)
            data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
        pv = _lib.PackedView()
        pv.data, pv.char_width, pv.n_rows, pv.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
        conv = torch.empty((n, 256), dtype=torch.uint8, device=dev)
        conv_len = torch.empty(n, dtype=torch.int32, device=dev)
        cv = _lib.BatchView()
        cv.rows, cv.char_width, cv.n_rows, cv.row_stride, cv.row_len, cv.lengths = conv.data_ptr(), 1, n, 256, 256, conv_len.data_ptr()
        rv = _lib.BatchView()
        rv.rows, rv.char_width, rv.n_rows, rv.row_stride, rv.row_len, rv.lengths = rows.data_ptr(), 1, n, 256, 256, l32.data_ptr()
        # the exact total first (one synchronising count), so that no timed step has to synchronise
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        check(L.needle_count_matches_packed_dev(h, ctypes.byref(pv), counts.data_ptr(), stream))
        m = int(counts.to(torch.int64).sum().item())
        c_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        c_se = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        c_tot = torch.zeros(1, dtype=torch.int64, device=dev)
        csr_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        st = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        en = torch.empty(max(m, 1), dtype=torch.int32, device=dev)

        def a_compact():
            check(L.needle_find_all_compact16_packed_dev(h, ctypes.byref(pv), mpr, c_off.data_ptr(), c_se.data_ptr(), m, c_tot.data_ptr(), None, stream))

        def a_csr():
            check(L.needle_count_matches_packed_dev(h, ctypes.byref(pv), counts.data_ptr(), stream))
            torch.cumsum(counts, 0, out=csr_off[1:])
            check(L.needle_find_all_csr_packed_dev(h, ctypes.byref(pv), csr_off.data_ptr(), st.data_ptr(), en.data_ptr(), None, stream))

        def convert():
            check(L.needle_rows_from_packed_dev(ctypes.byref(pv), conv.data_ptr(), 256, conv_len.data_ptr(), None, stream))

        def b_compact():
            convert()
            check(L.needle_find_all_compact16_dev(h, ctypes.byref(cv), mpr, c_off.data_ptr(), c_se.data_ptr(), m, c_tot.data_ptr(), None, stream))

        def b_csr():
            convert()
            check(L.needle_count_matches_dev(h, ctypes.byref(cv), counts.data_ptr(), stream))
            torch.cumsum(counts, 0, out=csr_off[1:])
            check(L.needle_find_all_csr_dev(h, ctypes.byref(cv), csr_off.data_ptr(), st.data_ptr(), en.data_ptr(), None, stream))

        def c_compact():
            check(L.needle_find_all_compact16_dev(h, ctypes.byref(rv), mpr, c_off.data_ptr(), c_se.data_ptr(), m, c_tot.data_ptr(), None, stream))

        routes = [("a", a_compact, True), ("a'", a_csr, False), ("b", b_compact, True), ("b'", b_csr, False), ("c", c_compact, True)]
        sums = {}
        for tag, fn, compact in routes:  # answers (one step each, buffers cleared first)
            (c_se if compact else st).fill_(0)
            if not compact:
                en.fill_(0)
            fn()
            torch.cuda.synchronize()
            if compact:
                t = int(c_tot.item())
                se = c_se[:t].to(torch.int64) & 0xFFFFFFFF
                sums[tag] = (t, int((se & 0xFFFF).sum().item()) + int((se >> 16).sum().item()))
            else:
                sums[tag] = (int(csr_off[-1].item()), int(st.to(torch.int64).sum().item()) + int(en.to(torch.int64).sum().item()))
        assert len(set(sums.values())) == 1, sums  # every route: the same matches (max_per_row is above every row's count here)
        steps = {tag: [] for tag, _, _ in routes}
        ev = {tag: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for tag, _, _ in routes}
        for r in range(args.warmup + args.steps):
            for tag, fn, _ in routes:
                e0, e1 = ev[tag]
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    steps[tag].append(e0.elapsed_time(e1))
        # the MEDIAN step (a step now and then takes 10-100x longer on the fixed-stride compact16 routes: the mean would report those)
        ms = {tag: sorted(v)[len(v) // 2] for tag, v in steps.items()}
        out = {"workload": wl, "what": what + ", per-row lengths uniform in [1, 256], packed", "transducer": {1: "lengths", 2: "run"}[kind],
               "rows": n, "chars": chars, "matches": sums["a"][0], "checksum_start_end": sums["a"][1], "max_per_row": mpr}
        for tag, _, compact in routes:
            res = (n * 8 + 8) + (m * 4 if compact else n * 4 + m * 8)
            actual = chars + n * 8 + res
            out[tag] = {"ms": round(ms[tag], 4), "ms_min": round(min(steps[tag]), 4), "ms_max": round(max(steps[tag]), 4), "GB/s": round(actual / ms[tag] / 1e6, 1),
                        "share_of_8TBs": round(actual / ms[tag] / 1e6 / HBM_PEAK_GBS, 4), "actual_bytes": actual, "checksum": sums[tag][1]}
        print(json.dumps(out), flush=True)
        del rows, data, conv, conv_len, c_se, st, en


if __name__ == "__main__":
    main()
