#!/usr/bin/env python3
"""A text buffer cut into lines on the device (needle_lines_count_packed_dev / needle_lines_fill_packed_dev) on bench.py's c2 text
(make_pattern / make_rows, per-row lengths (r * 2654435761) % 256 + 1) packed back to back: 1.285 GB for 10^7 rows.  Every row becomes a
LINE of 1..256 bytes: its last byte is made '\\n', every fourth line of two bytes or more ends in "\\r\\n"; no other terminator is left
in the text.  The buffer is split twice: as ONE document, and as 10^4 documents (cut at line ends, evenly by line number).
Stages, each between two HIP events, K steps a window, the stages ALTERNATED in one process, three windows each, the best one counts:
  count        needle_lines_count_packed_dev (STRIP: both counts)
  fill strip   needle_lines_fill_packed_dev: the line offsets and the compacted text
  fill keep    needle_lines_fill_packed_dev with NEEDLE_LINES_KEEP_ENDS: the line offsets only
  copy         dst.copy_(src) of as many bytes as the buffer holds -- the yardstick (count reads that many; fill strip reads them and
               writes nearly as many)
Before timing, the result is checked: one line per row, the kept units, the lines per document, and a sample of lines against slices
taken on the host.
python scripts/lines_rate.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--docs D]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--docs", type=int, default=10_000)
    args = ap.parse_args()
    import torch
    import bench
    from needle_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("lines_rate.py measures on the GPU: no device here, nothing measured")
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = args.rows
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    ends = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ends[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    chars = int(ends[-1].item())
    stream = torch.cuda.current_stream(dev).cuda_stream
    pattern, what, words = bench.make_pattern("c2")
    rows = bench.make_rows("c2", words, 0, n, dev)
    data = torch.zeros((chars + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
    for s in range(0, n, 1 << 20):  # packed slab by slab
        k = min(1 << 20, n - s)
        data[int(ends[s].item()):int(ends[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
    del rows, col
    for s in range(0, chars, 1 << 28):  # no terminator of the text's own
        part = data[s:min(chars, s + (1 << 28))]
        part[(part == 10) | (part == 13)] = 32
    data[ends[1:] - 1] = 10
    crlf = (torch.arange(n, device=dev) % 4 == 0) & (lens >= 2)
    data[ends[1:][crlf] - 2] = 13
    terminators = n + int(crlf.sum().item())
    del crlf
    units = chars  # data_units: the buffer's size as the caller knows it
    tiles = L.needle_lines_tiles(units, 1)
    tl = torch.empty(2 * tiles, dtype=torch.int64, device=dev)
    base = torch.zeros(2 * (tiles + 1), dtype=torch.int64, device=dev)
    lb, ub = base[:tiles + 1], base[tiles + 1:]
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out = torch.empty((chars + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
    src = torch.empty_like(out)

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

    for n_docs in (1, args.docs):
        cuts = torch.arange(n_docs + 1, device=dev, dtype=torch.int64) * n // n_docs
        doc_off = ends[cuts].contiguous()
        doc_lines = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        pv = _lib.PackedView()
        pv.data, pv.char_width, pv.n_rows, pv.offsets = data.data_ptr(), 1, n_docs, doc_off.data_ptr()

        def f_count():
            check(L.needle_lines_count_packed_dev(ctypes.byref(pv), units, 0, tl.data_ptr(), tl.data_ptr() + 8 * tiles, stream))

        def f_strip():
            check(L.needle_lines_fill_packed_dev(ctypes.byref(pv), units, 0, lb.data_ptr(), ub.data_ptr(), out_off.data_ptr(), out.data_ptr(),
                                                 doc_lines.data_ptr(), stream))

        def f_keep():
            check(L.needle_lines_fill_packed_dev(ctypes.byref(pv), units, _lib.LINES_KEEP_ENDS, lb.data_ptr(), None, out_off.data_ptr(), None,
                                                 doc_lines.data_ptr(), stream))

        def f_copy():
            out[:chars].copy_(src[:chars])

        # the answer first
        f_count()
        torch.cumsum(tl[:tiles], 0, out=lb[1:])
        torch.cumsum(tl[tiles:], 0, out=ub[1:])
        torch.cuda.synchronize()
        assert int(lb[-1].item()) == n and int(ub[-1].item()) == chars - terminators, (int(lb[-1].item()), int(ub[-1].item()))
        f_keep()
        torch.cuda.synchronize()
        assert torch.equal(out_off, ends) and torch.equal(doc_lines, cuts)
        f_strip()
        torch.cuda.synchronize()
        assert torch.equal(doc_lines, cuts) and int(out_off[-1].item()) == chars - terminators
        ho = out_off.cpu().numpy()
        for r in list(range(0, n, max(1, n // 2000)))[:2000] + [n - 1]:
            a, b = int(ends[r].item()), int(ends[r + 1].item())
            want = bytes(data[a:b].cpu().numpy()).rstrip(b"\r\n")
            assert bytes(out[int(ho[r]):int(ho[r + 1])].cpu().numpy()) == want, r
        del ho
        stages = [("count", f_count), ("fill_strip", f_strip), ("fill_keep", f_keep), ("copy", f_copy)]
        for _, fn in stages:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k, _ in stages}
        for _ in range(args.rounds):
            for k, fn in stages:
                ms[k].append(round(timed(fn), 4))
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps({"documents": n_docs, "what": "bench c2 text, lines of 1..256 bytes, a quarter of them ending in \\r\\n", "lines": n, "bytes": chars,
                          "tiles": int(tiles), "tile_units": int(L.needle_lines_tile_units(1)), "kept_bytes": chars - terminators, "ms_per_step": ms,
                          "best_ms": best, "count_GB/s_read": round(chars / best["count"] / 1e6, 1),
                          "fill_strip_GB/s_read_plus_written": round((2 * chars - terminators) / best["fill_strip"] / 1e6, 1),
                          "fill_keep_GB/s_read": round(chars / best["fill_keep"] / 1e6, 1),
                          "copy_GB/s_read_plus_written": round(2 * chars / best["copy"] / 1e6, 1),
                          "count_over_copy": round(best["count"] / best["copy"], 3), "fill_strip_over_copy": round(best["fill_strip"] / best["copy"], 3),
                          "fill_keep_over_copy": round(best["fill_keep"] / best["copy"], 3),
                          "count_plus_fill_strip_over_copy": round((best["count"] + best["fill_strip"]) / best["copy"], 3)}), flush=True)


if __name__ == "__main__":
    main()
