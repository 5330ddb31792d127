#!/usr/bin/env python3
"""Packed device batches: the direct scan (needle_*_packed_dev) against what such a batch cost before.  The rows are bench.py's c2r / c3r
rows (make_pattern / make_rows, per-row lengths (r * 2654435761) % 256 + 1), packed back to back on the device.  Per workload, K steps
between two HIP events after W warm-up steps:
  (a) direct     needle_{contained_in,find}_packed_dev on the packed batch
  (b) convert    needle_rows_from_packed_dev (stride 256, no sync) + the fixed-stride ragged call on its output
  (c) ragged     the fixed-stride ragged call on the 256-byte rows (bench.py's c2r / c3r)
GB/s over ACTUAL bytes: chars + 8 B offset per row + result bytes (bitmap, + 8 B start / end per row for find), fraction of 8 TB/s.
python scripts/packed_rate.py [--rows N] [--steps K] [--warmup W] [--only c2p|c3p] [--which a,b,c]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="c2p,c3p")
    ap.add_argument("--which", default="a,b,c")
    args = ap.parse_args()
    import torch
    import bench
    from needle_amd import _lib
    from needle_amd.pattern import unpack_bitmap
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = args.rows
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    l32 = lens.to(torch.int32)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    chars = int(offsets[-1].item())
    words_n = (n + 63) // 64
    for wl in args.only.split(","):
        base = {"c2p": "c2", "c3p": "c3"}[wl]
        is_find = base == "c3"
        pattern, what, words = bench.make_pattern(base)
        rows = bench.make_rows(base, words, 0, n, dev)
        data = torch.empty(chars, dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 20):  # packed slab by slab (one boolean mask over 2.56 G chars is beyond torch's indexing)
            k = min(1 << 20, n - s)
            data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
        bm = torch.empty(words_n, dtype=torch.int64, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev) if is_find else None
        en = torch.empty(n, dtype=torch.int32, device=dev) if is_find else None
        conv = torch.empty((n, 256), dtype=torch.uint8, device=dev)
        conv_len = torch.empty(n, dtype=torch.int32, device=dev)
        pv = _lib.PackedView()
        pv.data, pv.char_width, pv.n_rows, pv.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
        stream = torch.cuda.current_stream(dev).cuda_stream

        def direct():
            if is_find:
                pattern.find_packed(data, offsets, out=(bm, st, en))
            else:
                pattern.contained_in_packed(data, offsets, out=bm)

        def convert():
            rc = L.needle_rows_from_packed_dev(ctypes.byref(pv), conv.data_ptr(), 256, conv_len.data_ptr(), None, stream)
            assert rc == 0, L.needle_last_error()
            if is_find:
                pattern.find_batch(conv, conv_len, out=(bm, st, en))
            else:
                pattern.contained_in_batch(conv, conv_len, out=bm)

        def ragged():
            if is_find:
                pattern.find_batch(rows, l32, out=(bm, st, en))
            else:
                pattern.contained_in_batch(rows, l32, out=bm)
        actual = chars + n * 8 + words_n * 8 + (n * 8 if is_find else 0)
        results = {}
        for tag, fn in (("a", direct), ("b", convert), ("c", ragged)):
            if tag not in args.which.split(","):
                continue
            for _ in range(max(2, args.warmup)):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.steps
            res = {"ms_per_step": round(ms, 4), "GB/s": round(actual / ms / 1e6, 1), "frac_of_8TBs": round(actual / ms / 1e6 / HBM_PEAK_GBS, 4),
                   "matched": int(unpack_bitmap(bm, n).sum())}
            if is_find:
                res["checksum_start_end"] = int(st.to(torch.int64).sum().item()) + int(en.to(torch.int64).sum().item())
            results[tag] = res
        # the three routes must agree
        assert len({(r["matched"], r.get("checksum_start_end")) for r in results.values()}) == 1, results
        print(json.dumps({"workload": wl, "what": what + ", per-row lengths uniform in [1, 256], packed", "rows": n, "chars": chars,
                          "actual_bytes": actual, "a_direct": results.get("a"), "b_convert_then_fixed": results.get("b"),
                          "c_fixed_stride_ragged": results.get("c")}), flush=True)
        del rows, data, conv, conv_len, bm, st, en


if __name__ == "__main__":
    main()
