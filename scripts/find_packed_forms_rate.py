#!/usr/bin/env python3
"""find() result forms of packed device batches: what the 16- and 8-bit forms (needle_find_packed{16,8}_packed_dev) cost against the
int32 pairs (needle_find_packed_dev), on the device and landed in host memory.  The rows are packed_rate.py's c2p / c3p batches (bench.py's
c2 / c3 rows, per-row lengths (r * 2654435761) % 256 + 1, packed back to back on the device); both are run through find().  Per workload,
medians over K steps of HIP events after W warm-up steps:
  kernel      the _dev call alone, per form (int32 | 16 | 8), and needle_find_next_packed_dev from cursor 0
  landed      the _dev call + the copy of bitmap and results into pinned host memory, per form
  host        the _host entries end to end on the same packed arrays in (pageable) host memory: needle_find_packed_host (converts to
              fixed-stride rows on the device) against needle_find_packed{16,8}_packed_host (direct packed kernel)
python scripts/find_packed_forms_rate.py [--rows N] [--steps K] [--warmup W] [--only c2p,c3p] [--host-steps H]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--only", default="c2p,c3p")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from needle_amd.pattern import unpack_bitmap
    dev = torch.device("cuda", 0)
    n = args.rows
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    chars = int(offsets[-1].item())
    nw = (n + 63) // 64
    for wl in args.only.split(","):
        base = {"c2p": "c2", "c3p": "c3"}[wl]
        pattern, what, words = bench.make_pattern(base)
        rows = bench.make_rows(base, words, 0, n, dev)
        data = torch.empty(chars, dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 20):
            k = min(1 << 20, n - s)
            data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
        del rows
        bm = torch.empty(nw, dtype=torch.int64, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        en = torch.empty(n, dtype=torch.int32, device=dev)
        r16 = torch.empty(n, dtype=torch.int32, device=dev)
        r8 = torch.empty(n, dtype=torch.int16, device=dev)
        ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        h_bm = torch.empty(nw, dtype=torch.int64, pin_memory=True)
        h_st = torch.empty(n, dtype=torch.int32, pin_memory=True)
        h_en = torch.empty(n, dtype=torch.int32, pin_memory=True)
        h_r16 = torch.empty(n, dtype=torch.int32, pin_memory=True)
        h_r8 = torch.empty(n, dtype=torch.int16, pin_memory=True)
        kern = {"int32": lambda: pattern.find_packed(data, offsets, out=(bm, st, en)),
                "16": lambda: pattern.find_packed16_packed(data, offsets, out=(bm, r16, ovf)),
                "8": lambda: pattern.find_packed8_packed(data, offsets, out=(bm, r8, ovf))}
        copies = {"int32": lambda: (h_bm.copy_(bm, non_blocking=True), h_st.copy_(st, non_blocking=True), h_en.copy_(en, non_blocking=True)),
                  "16": lambda: (h_bm.copy_(bm, non_blocking=True), h_r16.copy_(r16, non_blocking=True)),
                  "8": lambda: (h_bm.copy_(bm, non_blocking=True), h_r8.copy_(r8, non_blocking=True))}

        def median_ms(fn):
            for _ in range(max(2, args.warmup)):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            return round(statistics.median(ts), 4)
        out = {"workload": wl, "what": what + ", run as find(); per-row lengths uniform in [1, 256], packed", "rows": n, "chars": chars}
        for form in ("int32", "16", "8"):
            out["kernel_ms_" + form] = median_ms(kern[form])
            out["landed_ms_" + form] = median_ms(lambda: (kern[form](), copies[form]()))
        out["result_bytes"] = {"int32": nw * 8 + n * 8, "16": nw * 8 + n * 4, "8": nw * 8 + n * 2}
        # the cursor entry from cursor 0 (the same answers as the int32 entry; its kernels use 64-byte windows only)
        cur0 = torch.zeros(n, dtype=torch.int32, device=dev)
        out["kernel_ms_next_cursor0"] = median_ms(lambda: pattern.find_next_packed(data, offsets, cur0))
        # the forms agree with the int32 pairs (every row of these batches fits both forms)
        pattern.find_packed(data, offsets, out=(bm, st, en))
        torch.cuda.synchronize()
        bm_ref = bm.clone()
        ovf.zero_()
        pattern.find_packed16_packed(data, offsets, out=(bm, r16, ovf))
        want16 = torch.where(en < 0, torch.full_like(en, -1), (st & 0xFFFF) | (en << 16))
        torch.cuda.synchronize()
        assert torch.equal(bm, bm_ref) and torch.equal(r16, want16) and int(ovf.item()) == 0
        pattern.find_packed8_packed(data, offsets, out=(bm, r8, ovf))
        ln = en - st
        want8 = torch.where(en < 0, torch.full_like(en, 0xFFFF), torch.where(ln > 255, torch.full_like(ln, 0xFFFE), (st & 0xFF) | (ln << 8)))
        torch.cuda.synchronize()
        assert torch.equal(bm, bm_ref) and torch.equal(r8.to(torch.int32) & 0xFFFF, want8) and int(ovf.item()) == 0
        out["matched"] = int(unpack_bitmap(bm_ref, n).sum())
        # host entries end to end (numpy arrays in pageable memory)
        hd, ho = data.cpu().numpy(), offsets.cpu().numpy()
        for tag, fn in (("host_ms_find_packed_host", lambda: pattern.find_packed(hd, ho)),
                        ("host_ms_16_packed_host", lambda: pattern.find_packed16_packed(hd, ho)),
                        ("host_ms_8_packed_host", lambda: pattern.find_packed8_packed(hd, ho))):
            fn()
            ts = []
            for _ in range(args.host_steps):
                t0 = time.perf_counter()
                r = fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[tag] = round(statistics.median(ts), 2)
            assert (np.asarray(r[0]).view(np.int64)[:nw] == bm_ref.cpu().numpy()).all(), tag
        print(json.dumps(out), flush=True)
        del data, bm, st, en, r16, r8


if __name__ == "__main__":
    main()
