#!/usr/bin/env python3
"""Equal spans put into groups (needle_group_spans_packed_dev: hash, insert, finish) on bench.py's c2 / c3 rows (make_pattern / make_rows,
per-row lengths (r * 2654435761) % 256 + 1), packed back to back on the device, on two lists:
  c3 matches   the 1000-keyword union's find-all list: tens of millions of spans, about 1000 distinct -- the hot-key case
  c2 matches   `[0-9]+`'s find-all list: digit runs, mostly distinct
Stages, each between two HIP events, K steps a window, the stages ALTERNATED in one process, R windows each, the median step counts:
  group     needle_group_spans_packed_dev: the table's hipMemsetAsync and the three kernels
  clear     the same hipMemsetAsync alone (torch zero_ of as many bytes as the entry clears)
  copy      dst.copy_(src) of as many bytes as the spans hold -- the yardstick (the hash pass reads that many bytes of text once, the
            insert pass once more per comparison)
  lengths   needle_gather_spans_lengths_packed_dev on the same list: the skeleton alone (offsets, row search, clamp, one store per span)
  set_spans needle_set_matches_spans_packed_dev on the same list with the 32-keyword set of tests/pattern_set_cases.py (KW32: one group,
            an 8-bit table): the sibling kernel -- one lane per span, the same aligned block loads of the span's text, a table walk
            where the hash pass folds (profiles/set_spans.md has it on its own list)
--passes    the three kernels apart: per workload a child process of this script (5 steps, no host part) under a kernel trace (rocprofv3
            --kernel-trace --output-format csv), the medians of group_hash_kernel / group_insert_kernel / group_finish_kernel read off
            the trace; printed as one more JSON line per workload, with the insert pass per span
host        the alternative without the entry, at --host-rows rows: gather_spans_packed + download + a Python dict over the slices (wall
            clock, one run) beside distinct_spans_packed + download of the table on the same rows
Before timing, the result is compared with a dict built on the host on a sample batch (--host-rows rows).
python scripts/group_rate.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--only c3,c2] [--host-rows H] [--passes]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def traced_passes(args, wl):
    """The kernels of one workload apart: a fresh child of this script under a kernel trace -> {kernel: median ms}, spans."""
    import csv
    import glob
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "group", "--", sys.executable, os.path.abspath(__file__),
               "--rows", str(args.rows), "--steps", "5", "--rounds", "1", "--warmup", "1", "--only", wl, "--host-rows", "1000"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        spans = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1])["spans"]
        took = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    for k in ("group_hash", "group_insert", "group_finish"):
                        if k + "_kernel" in row["Kernel_Name"]:
                            took.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    # (the launches on the whole list; the sample batch's are a hundredth of them)
    return {k: statistics.median([x for x in v if x > max(v) / 4]) for k, v in took.items()}, spans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="c3,c2")
    ap.add_argument("--host-rows", type=int, default=200_000)
    ap.add_argument("--passes", action="store_true")
    args = ap.parse_args()
    if args.passes:  # (before this process opens the device: the children run one after the other)
        for wl in args.only.split(","):
            ms, spans = traced_passes(args, wl)
            print(json.dumps({"workload": wl, "spans": spans, "kernel_median_ms": {k: round(v, 4) for k, v in ms.items()},
                              "ns_per_span": {k: round(v * 1e6 / max(spans, 1), 4) for k, v in ms.items()}}), flush=True)
    import numpy as np
    import torch
    import bench
    from needle_amd import _lib
    from needle_amd.pattern import DFACompiler, Pattern, PatternSet
    from pattern_set_cases import KW32
    if not torch.cuda.is_available():
        raise SystemExit("group_rate.py measures on the GPU: no device here, nothing measured")
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = args.rows
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    chars = int(offsets[-1].item())
    stream = torch.cuda.current_stream(dev).cuda_stream
    kw32 = PatternSet([DFACompiler.compile(w, "w%d" % i) for i, w in enumerate(KW32)])

    def check(rc):
        assert rc == 0, L.needle_last_error()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    for wl in args.only.split(","):
        pattern, what, words = bench.make_pattern(wl)
        rows = bench.make_rows(wl, words, 0, n, dev)
        data = torch.empty((chars + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 20):  # packed slab by slab
            k = min(1 << 20, n - s)
            data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
        del rows
        pv = _lib.PackedView()
        pv.data, pv.char_width, pv.n_rows, pv.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
        moff, st, en = pattern.find_all_packed(data, offsets)
        m = st.numel()

        # ---- the answer on the first --host-rows rows against a dict built on the host, and the two end-to-end alternatives there
        h = min(args.host_rows, n)
        hoff = offsets[:h + 1].contiguous()
        hm = int(moff[h].item())
        hmo, hst, hen = moff[:h + 1].contiguous(), st[:hm].contiguous(), en[:hm].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        text, toff = Pattern.gather_spans_packed(data, hoff, hmo, hst, hen)
        host_text, host_off = text.cpu().numpy().tobytes(), toff.cpu().numpy()
        table = {}
        for k in range(hm):
            key = host_text[host_off[k]:host_off[k + 1]]
            table[key] = table.get(key, 0) + 1
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        dtext, doff, dcounts, _ = Pattern.distinct_spans_packed(data, hoff, hmo, hst, hen)
        dtext, doff, dcounts = dtext.cpu().numpy().tobytes(), doff.cpu().numpy(), dcounts.cpu().numpy()
        t_dev = time.perf_counter() - t0
        got = [(dtext[doff[g]:doff[g + 1]], int(dcounts[g])) for g in range(dcounts.size)]
        assert got == list(table.items()), (wl, "the device's table differs from the host's dict")
        del text, toff

        # ---- the entry on the whole list
        work_bytes = int(L.needle_group_spans_work_bytes(m))
        work = torch.empty((work_bytes + 7) // 8, dtype=torch.int64, device=dev)
        first = torch.empty(m + 1, dtype=torch.int64, device=dev)
        count = torch.empty(m + 1, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out_len = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        slots = 64
        while slots < 2 * m:
            slots *= 2
        table_words = torch.empty(2 * slots, dtype=torch.int32, device=dev)

        def f_group():
            check(L.needle_group_spans_packed_dev(ctypes.byref(pv), moff.data_ptr(), st.data_ptr(), en.data_ptr(), m, 64, work.data_ptr(), work_bytes,
                                                  first.data_ptr(), count.data_ptr(), status.data_ptr(), stream))

        def f_clear():
            table_words.zero_()

        def f_lengths():
            check(L.needle_gather_spans_lengths_packed_dev(ctypes.byref(pv), moff.data_ptr(), st.data_ptr(), en.data_ptr(), out_len.data_ptr(), stream))

        masks = torch.empty(m + 1, dtype=torch.int32, device=dev)

        def f_set_spans():
            kw32.matches_spans_packed(data, offsets, moff, st, en, out=masks)

        f_group()
        f_lengths()
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        span_bytes = int(out_len[:m].sum().item())
        leaders = int((first[:m] == torch.arange(m, device=dev)).sum().item())
        biggest = int(count[:m].max().item()) if m else 0
        src = torch.empty(span_bytes + 4, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def f_copy():
            dst.copy_(src)

        stages = [("group", f_group), ("clear", f_clear), ("copy", f_copy), ("lengths", f_lengths), ("set_spans", f_set_spans)]
        for _, fn in stages:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k, _ in stages}
        for _ in range(args.rounds):
            for k, fn in stages:
                ms[k].append(round(timed(fn), 4))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"workload": wl, "what": what + ", per-row lengths uniform in [1, 256], packed", "rows": n, "chars": chars, "spans": m,
                          "span_bytes": span_bytes, "distinct": leaders, "largest_group": biggest, "slots": slots, "work_bytes": work_bytes,
                          "ms_per_step": ms, "median_ms": med, "group_ns_per_span": round(med["group"] * 1e6 / max(m, 1), 3),
                          "group_minus_clear_ns_per_span": round((med["group"] - med["clear"]) * 1e6 / max(m, 1), 3),
                          "group_over_copy": round(med["group"] / med["copy"], 2), "group_over_set_spans": round(med["group"] / med["set_spans"], 2), "host_rows": h, "host_spans": hm, "host_distinct": len(table),
                          "host_gather_download_dict_s": round(t_host, 3), "device_distinct_spans_download_s": round(t_dev, 4)}), flush=True)
        del data, moff, st, en, work, first, count, out_len, table_words, src, dst, masks


if __name__ == "__main__":
    main()
