#!/usr/bin/env python3
"""Replace every match of every packed row (needle_replace_all_lengths_packed_dev / needle_replace_all_fill_packed_dev) beside the find-all
passes it builds on, and its fill kernel against a plain device-to-device copy of the same number of output bytes.  The rows are bench.py's
c2 / c3 rows (make_pattern / make_rows, per-row lengths (r * 2654435761) % 256 + 1), packed back to back on the device:
  c2  `[0-9]+` -> "#"       c3  the 1000-keyword union -> "***"
Stages, each between two HIP events, K steps a window, the stages ALTERNATED in one process, three windows each, the best one counts:
  count     needle_count_matches_packed_dev
  csr       needle_find_all_csr_packed_dev
  lengths   needle_replace_all_lengths_packed_dev
  cumsums   the two torch.cumsum calls (match counts, output lengths)
  fill      needle_replace_all_fill_packed_dev
  copy      dst.copy_(src) of as many bytes as fill writes -- the yardstick
  all       the five in sequence (no host read: the totals are known from a first run)
Reported besides: the fill kernel's read + written bytes over its time, fill / copy, the splice kernels' share of the end-to-end replace,
and the share of the fill kernel's 16-byte steps that take its unit-by-unit path (those that hold a replacement byte or the seam of two
gaps), computed from the match list.  Before timing, the result is compared with a torch splice of the same list on a sample of rows.
python scripts/replace_rate.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--only c2,c3]"""
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
        raise SystemExit("replace_rate.py measures on the GPU: no device here, nothing measured")
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
        h = pattern._h
        repl = Pattern._repl_units(REPL[wl], 1)
        R = int(repl.size)
        rows = bench.make_rows(wl, words, 0, n, dev)
        data = torch.empty((chars + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 20):  # packed slab by slab
            k = min(1 << 20, n - s)
            data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
        del rows
        pv = _lib.PackedView()
        pv.data, pv.char_width, pv.n_rows, pv.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
        # a first run through the public composition: the totals, and the buffers every timed step reuses
        out_text, out_off_first = pattern.replace_all_packed(data, offsets, REPL[wl])
        torch.cuda.synchronize()
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        moff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        check(L.needle_count_matches_packed_dev(h, ctypes.byref(pv), counts.data_ptr(), stream))
        torch.cumsum(counts, 0, out=moff[1:])
        m = int(moff[-1].item())
        st = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        en = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        out_len = torch.empty(n, dtype=torch.int64, device=dev)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = int(out_off_first[-1].item())
        out = torch.empty((total + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
        src = torch.empty_like(out)

        def f_count():
            check(L.needle_count_matches_packed_dev(h, ctypes.byref(pv), counts.data_ptr(), stream))

        def f_csr():
            check(L.needle_find_all_csr_packed_dev(h, ctypes.byref(pv), moff.data_ptr(), st.data_ptr(), en.data_ptr(), None, stream))

        def f_lengths():
            check(L.needle_replace_all_lengths_packed_dev(ctypes.byref(pv), moff.data_ptr(), st.data_ptr(), en.data_ptr(), R, out_len.data_ptr(), stream))

        def f_cumsums():
            torch.cumsum(counts, 0, out=moff[1:])
            torch.cumsum(out_len, 0, out=out_off[1:])

        def f_fill():
            check(L.needle_replace_all_fill_packed_dev(ctypes.byref(pv), moff.data_ptr(), st.data_ptr(), en.data_ptr(), repl.ctypes.data, R,
                                                       out_off.data_ptr(), out.data_ptr(), stream))

        def f_copy():
            out[:total].copy_(src[:total])

        def f_all():
            f_count()
            torch.cumsum(counts, 0, out=moff[1:])
            f_csr()
            f_lengths()
            torch.cumsum(out_len, 0, out=out_off[1:])
            f_fill()

        f_all()
        torch.cuda.synchronize()
        assert int(out_off[-1].item()) == total and torch.equal(out_off, out_off_first) and torch.equal(out[:total], out_text)
        # the answer on a sample of rows against a splice done with torch on the host
        hs, he, hm = st.cpu().numpy(), en.cpu().numpy(), moff.cpu().numpy()
        for r in list(range(0, n, max(1, n // 2000)))[:2000]:
            a, b = int(offsets[r].item()), int(offsets[r + 1].item())
            row = data[a:b].cpu().numpy()
            parts, pos = [], 0
            for k in range(hm[r], hm[r + 1]):
                parts += [row[pos:hs[k]], repl]
                pos = he[k]
            want = np.concatenate(parts + [row[pos:]])
            got = out[int(out_off[r].item()):int(out_off[r + 1].item())].cpu().numpy()
            assert got.size == want.size and (got == want).all(), (wl, r)
        # the 16-byte steps of the fill kernel that take the unit-by-unit path: those that hold a replacement byte or the seam of two gaps
        row_of = torch.repeat_interleave(torch.arange(n, device=dev), counts.to(torch.int64))
        s64, e64 = st[:m].to(torch.int64), en[:m].to(torch.int64)
        delta = R - (e64 - s64)
        o_m = offsets[row_of] - offsets[0] + s64 + torch.cumsum(delta, 0) - delta  # output byte of replacement m (out_offsets[0] = 0, 16-byte aligned buffer)
        assert out.data_ptr() % 16 == 0 and R <= 16
        n_blocks = (total + 15) // 16
        slow = torch.zeros(n_blocks + 1, dtype=torch.bool, device=dev)
        if R:
            slow[o_m // 16] = True
            slow[(o_m + R - 1) // 16] = True
        else:
            slow[(o_m // 16)[o_m % 16 != 0]] = True
        slow_share = float(slow[:n_blocks].sum().item()) / max(n_blocks, 1)
        del row_of, s64, e64, delta, o_m, slow
        stages = [("count", f_count), ("csr", f_csr), ("lengths", f_lengths), ("cumsums", f_cumsums), ("fill", f_fill), ("copy", f_copy), ("all", f_all)]
        for _, fn in stages:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in stages}
        for _ in range(args.rounds):
            for name, fn in stages:
                ms[name].append(round(timed(fn), 4))
        best = {k: min(v) for k, v in ms.items()}
        fill_bytes = (chars + total) + m * 8 + 3 * (n + 1) * 8  # text read + written, the match list, the three offset arrays
        parts = best["count"] + best["csr"] + best["lengths"] + best["cumsums"] + best["fill"]
        print(json.dumps({"workload": wl, "what": what + ", per-row lengths uniform in [1, 256], packed", "replacement": REPL[wl], "rows": n, "chars": chars,
                          "matches": m, "out_chars": total, "ms_per_step": ms, "best_ms": best,
                          "fill_GB/s": round(fill_bytes / best["fill"] / 1e6, 1), "fill_bytes": fill_bytes,
                          "copy_GB/s_read_plus_written": round(2 * total / best["copy"] / 1e6, 1),
                          "fill_over_copy": round(best["fill"] / best["copy"], 3), "slow_path_share_of_16B_steps": round(slow_share, 4),
                          "splice_share_of_replace": round((best["lengths"] + best["fill"]) / parts, 3),
                          "sum_of_stages_ms": round(parts, 4)}), flush=True)
        del data, out, src, st, en, counts, moff, out_len, out_off, out_text, out_off_first


if __name__ == "__main__":
    main()
