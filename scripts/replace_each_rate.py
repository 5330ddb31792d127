#!/usr/bin/env python3
"""A replacement per match (needle_replace_each_lengths_packed_dev / needle_replace_each_fill_packed_dev) beside the plain replace-all
kernels, on the batch of scripts/replace_rate.py: bench.py's c2 / c3 rows, per-row lengths (r * 2654435761) % 256 + 1, packed back to
back on the device; the match list is find_all_packed's.
Stages, each between two HIP events, K steps a window, the stages ALTERNATED in one process, three windows each, the best one counts:
  plain_fill     (a) needle_replace_all_fill_packed_dev, c2 -> "#", c3 -> "***": the parent's kernel, untouched
  each_fill_1    (b) needle_replace_each_fill_packed_dev with that one entry and every choice 0: the same output (compared before timing)
  each_fill_32   (c) c3 only: a 32-entry table of lengths 0 .. 8 (entry i: i % 9 bytes), a quarter of the matches kept (choice -1)
  plain_lengths      needle_replace_all_lengths_packed_dev
  each_lengths_1 (d) needle_replace_each_lengths_packed_dev, one entry, every choice 0
  each_lengths_32    c3 only: the table and the choices of (c)
Before timing, (c)'s result is compared with a splice done on the host on a sample of rows.
python scripts/replace_each_rate.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--only c2,c3]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPL = {"c2": "#", "c3": "***"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="c2,c3")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from needle_amd import _lib
    from needle_amd.pattern import Pattern
    if not torch.cuda.is_available():
        raise SystemExit("replace_each_rate.py measures on the GPU: no device here, nothing measured")
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = args.rows
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    chars = int(offsets[-1].item())
    stream = torch.cuda.current_stream(dev).cuda_stream

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
        m = int(st.numel())
        # (a) and (b): one replacement
        repl = Pattern._repl_units(REPL[wl], 1)
        roff1 = np.array([0, repl.size], np.uint32)
        zero = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
        plain_text, plain_off = Pattern.splice_packed(data, offsets, moff, st, en, repl)
        each_text, each_off = Pattern.splice_each_packed(data, offsets, moff, st, en, zero[:m], [repl])
        torch.cuda.synchronize()
        assert torch.equal(plain_off, each_off) and torch.equal(plain_text, each_text), "one entry, every choice 0: replace all"
        total1 = int(plain_off[-1].item())
        out1 = torch.empty((total1 + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
        out_len = torch.empty(n, dtype=torch.int64, device=dev)
        del each_text, each_off, plain_text
        A = (ctypes.byref(pv), moff.data_ptr(), st.data_ptr(), en.data_ptr())

        def f_plain_fill():
            check(L.needle_replace_all_fill_packed_dev(*A, repl.ctypes.data, repl.size, plain_off.data_ptr(), out1.data_ptr(), stream))

        def f_each_fill_1():
            check(L.needle_replace_each_fill_packed_dev(*A, zero.data_ptr(), 0, repl.ctypes.data, roff1.ctypes.data, 1, plain_off.data_ptr(), out1.data_ptr(), stream))

        def f_plain_lengths():
            check(L.needle_replace_all_lengths_packed_dev(*A, repl.size, out_len.data_ptr(), stream))

        def f_each_lengths_1():
            check(L.needle_replace_each_lengths_packed_dev(*A, zero.data_ptr(), 0, roff1.ctypes.data, 1, out_len.data_ptr(), stream))

        stages = [("plain_fill", f_plain_fill), ("each_fill_1", f_each_fill_1), ("plain_lengths", f_plain_lengths), ("each_lengths_1", f_each_lengths_1)]
        extra = {}
        if wl == "c3":  # (c): 32 entries of 0 .. 8 bytes, a quarter of the matches kept
            table = [np.frombuffer((b"%02d:abcdef" % i)[:i % 9], np.uint8) for i in range(32)]
            r32, roff32 = Pattern._repl_table(table, 1)
            g = torch.Generator(device=dev)
            g.manual_seed(32)
            choice = torch.randint(0, 32, (max(m, 1),), generator=g, device=dev, dtype=torch.int32)
            choice[torch.rand(max(m, 1), generator=g, device=dev) < 0.25] = -1
            text32, off32 = Pattern.splice_each_packed(data, offsets, moff, st, en, choice[:m], table)
            torch.cuda.synchronize()
            total32 = int(off32[-1].item())
            hs, he, hm, hc = st.cpu().numpy(), en.cpu().numpy(), moff.cpu().numpy(), choice.cpu().numpy()
            for r in list(range(0, n, max(1, n // 2000)))[:2000]:  # a sample of rows against a splice on the host
                a, b = int(offsets[r].item()), int(offsets[r + 1].item())
                row = data[a:b].cpu().numpy()
                parts, pos = [], 0
                for k in range(hm[r], hm[r + 1]):
                    parts += [row[pos:hs[k]], table[hc[k]] if hc[k] >= 0 else row[hs[k]:he[k]]]
                    pos = he[k]
                want = np.concatenate(parts + [row[pos:]])
                got = text32[int(off32[r].item()):int(off32[r + 1].item())].cpu().numpy()
                assert got.size == want.size and (got == want).all(), (wl, r)
            out32 = torch.empty((total32 + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
            del text32

            def f_each_fill_32():
                check(L.needle_replace_each_fill_packed_dev(*A, choice.data_ptr(), 0, r32.ctypes.data, roff32.ctypes.data, 32, off32.data_ptr(), out32.data_ptr(),
                                                            stream))

            def f_each_lengths_32():
                check(L.needle_replace_each_lengths_packed_dev(*A, choice.data_ptr(), 0, roff32.ctypes.data, 32, out_len.data_ptr(), stream))

            stages += [("each_fill_32", f_each_fill_32), ("each_lengths_32", f_each_lengths_32)]
            extra = {"out_chars_32": total32, "kept_share_32": round(float((choice[:m] < 0).float().mean().item()), 4),
                     "each_fill_32_bytes": chars + total32 + m * 12 + 3 * (n + 1) * 8}
        for _, fn in stages:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in stages}
        for _ in range(args.rounds):
            for name, fn in stages:
                ms[name].append(round(timed(fn), 4))
        best = {k: min(v) for k, v in ms.items()}
        plain_bytes = chars + total1 + m * 8 + 3 * (n + 1) * 8   # text read + written, the match list, the three offset arrays
        each_bytes = plain_bytes + m * 4                         # ... and the choices
        res = {"workload": wl, "what": what + ", per-row lengths uniform in [1, 256], packed", "replacement": REPL[wl], "rows": n, "chars": chars,
               "matches": m, "out_chars": total1, "ms_per_step": ms, "best_ms": best, "plain_fill_bytes": plain_bytes, "each_fill_1_bytes": each_bytes,
               "plain_fill_GB/s": round(plain_bytes / best["plain_fill"] / 1e6, 1), "each_fill_1_GB/s": round(each_bytes / best["each_fill_1"] / 1e6, 1),
               "each_fill_1_over_plain_fill": round(best["each_fill_1"] / best["plain_fill"], 3),
               "each_lengths_1_over_plain_lengths": round(best["each_lengths_1"] / best["plain_lengths"], 3)}
        if extra:
            res.update(extra)
            res["each_fill_32_GB/s"] = round(extra["each_fill_32_bytes"] / best["each_fill_32"] / 1e6, 1)
        print(json.dumps(res), flush=True)
        del data, out1, st, en, moff, out_len, zero, plain_off


if __name__ == "__main__":
    main()
