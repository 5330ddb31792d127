#!/usr/bin/env python3
"""Spans of packed rows gathered into a new packed batch (needle_gather_spans_lengths_packed_dev / needle_gather_spans_fill_packed_dev,
needle_split_spans_packed_dev) on bench.py's c2 / c3 rows (make_pattern / make_rows, per-row lengths (r * 2654435761) % 256 + 1), packed
back to back on the device, on three lists:
  c2 matches   `[0-9]+`'s find-all list                       c3 matches   the 1000-keyword union's list: short spans, many per 16-byte block
  c3 pieces    the split list of c3's matches: long spans     c3 select    the rows contained_in_packed selects, whole (Pattern.select_rows_packed)
Stages, each between two HIP events, K steps a window, the stages ALTERNATED in one process, three windows each, the best one counts:
  lengths   needle_gather_spans_lengths_packed_dev            split     needle_split_spans_packed_dev (pieces only)
  fill      needle_gather_spans_fill_packed_dev
  copy      dst.copy_(src) of as many bytes as fill writes -- the yardstick (fill reads and writes that many bytes of text)
  replace   needle_replace_all_fill_packed_dev with a one-unit replacement on the SAME list -- the sibling sweep
  select    Pattern.select_rows_packed end to end (torch list building, lengths, cumsum, fill, one host read; c3 select only)
Reported besides: the pieces per 16-byte output block and the rounds per 64-block step (the most pieces of its blocks) that the list
implies, computed from the output offsets.  Before timing, the result is compared with slices taken on the host on a sample of spans.
python scripts/gather_rate.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--only c2,c3]"""
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
    ap.add_argument("--only", default="c2,c3")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from needle_amd import _lib
    from needle_amd.pattern import Pattern
    if not torch.cuda.is_available():
        raise SystemExit("gather_rate.py measures on the GPU: no device here, nothing measured")
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = args.rows
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    chars = int(offsets[-1].item())
    stream = torch.cuda.current_stream(dev).cuda_stream
    repl = Pattern._repl_units("#", 1)

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
        lists = [("matches", moff, st, en)]
        if wl == "c3":
            lists.append(("pieces",) + Pattern.split_spans_packed(data, offsets, moff, st, en))
        for name, so, ls, le in lists:
            m = ls.numel()
            # a first run through the public composition: the totals, and the buffers every timed step reuses
            text_first, off_first = Pattern.gather_spans_packed(data, offsets, so, ls, le)
            torch.cuda.synchronize()
            total = int(off_first[-1].item())
            out_len = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            out_off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            out = torch.empty((total + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
            src = torch.empty_like(out)
            po = torch.empty(n + 1, dtype=torch.int64, device=dev)
            pse = torch.empty(2 * (st.numel() + n) + 1, dtype=torch.int32, device=dev)
            # the replace sweep on the same list: its own lengths and offsets
            r_len = torch.empty(n, dtype=torch.int64, device=dev)
            r_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            check(L.needle_replace_all_lengths_packed_dev(ctypes.byref(pv), so.data_ptr(), ls.data_ptr(), le.data_ptr(), 1, r_len.data_ptr(), stream))
            torch.cumsum(r_len, 0, out=r_off[1:])
            r_total = int(r_off[-1].item())
            r_out = torch.empty((r_total + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)

            def f_lengths():
                check(L.needle_gather_spans_lengths_packed_dev(ctypes.byref(pv), so.data_ptr(), ls.data_ptr(), le.data_ptr(), out_len.data_ptr(), stream))

            def f_fill():
                check(L.needle_gather_spans_fill_packed_dev(ctypes.byref(pv), so.data_ptr(), ls.data_ptr(), le.data_ptr(), out_off.data_ptr(), out.data_ptr(),
                                                            stream))

            def f_copy():
                out[:total].copy_(src[:total])

            def f_replace():
                check(L.needle_replace_all_fill_packed_dev(ctypes.byref(pv), so.data_ptr(), ls.data_ptr(), le.data_ptr(), repl.ctypes.data, 1,
                                                           r_off.data_ptr(), r_out.data_ptr(), stream))

            def f_split():
                check(L.needle_split_spans_packed_dev(ctypes.byref(pv), moff.data_ptr(), st.data_ptr(), en.data_ptr(), po.data_ptr(), pse.data_ptr(),
                                                      pse.data_ptr() + 4 * (st.numel() + n), stream))

            f_lengths()
            torch.cumsum(out_len[:m], 0, out=out_off[1:])
            f_fill()
            torch.cuda.synchronize()
            assert torch.equal(out_off, off_first) and torch.equal(out[:total], text_first)
            # the answer on a sample of spans against slices taken on the host
            hso, hs, he, ho = so.cpu().numpy(), ls.cpu().numpy(), le.cpu().numpy(), out_off.cpu().numpy()
            for k in list(range(0, m, max(1, m // 2000)))[:2000]:
                r = int(np.searchsorted(hso, k, side="right")) - 1
                a, b = int(offsets[r].item()), int(offsets[r + 1].item())
                s0 = min(max(int(hs[k]), 0), b - a)
                e0 = min(max(int(he[k]), s0), b - a)
                want = data[a + s0:a + e0].cpu().numpy()
                got = out[int(ho[k]):int(ho[k + 1])].cpu().numpy()
                assert got.size == want.size and (got == want).all(), (wl, name, k)
            # pieces per 16-byte output block: +1 over the blocks every non-empty span touches (a difference array), then per 64-block step
            nb = (total + 15) // 16
            o0, o1 = out_off[:-1], out_off[1:]
            some = o1 > o0
            diff = torch.zeros(nb + 2, dtype=torch.int32, device=dev)
            diff.index_add_(0, (o0[some] // 16), torch.ones(int(some.sum().item()), dtype=torch.int32, device=dev))
            diff.index_add_(0, ((o1[some] - 1) // 16 + 1), -torch.ones(int(some.sum().item()), dtype=torch.int32, device=dev))
            per_block = torch.cumsum(diff, 0)[:nb]
            pad = torch.zeros((-nb) % 64, dtype=per_block.dtype, device=dev)
            per_step = torch.cat([per_block, pad]).view(-1, 64).max(dim=1).values
            pieces_per_block = float(per_block.float().mean().item()) if nb else 0.0
            rounds_per_step = float(per_step.float().mean().item()) if nb else 0.0
            del diff, per_block, per_step, some, hso, hs, he, ho
            stages = [("lengths", f_lengths), ("fill", f_fill), ("copy", f_copy), ("replace", f_replace)]
            if name == "pieces":
                stages.append(("split", f_split))
            for _, fn in stages:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k, _ in stages}
            for _ in range(args.rounds):
                for k, fn in stages:
                    ms[k].append(round(timed(fn), 4))
            best = {k: min(v) for k, v in ms.items()}
            print(json.dumps({"workload": wl, "list": name, "what": what + ", per-row lengths uniform in [1, 256], packed", "rows": n, "chars": chars,
                              "spans": m, "out_chars": total, "ms_per_step": ms, "best_ms": best,
                              "fill_GB/s_read_plus_written": round(2 * total / best["fill"] / 1e6, 1),
                              "copy_GB/s_read_plus_written": round(2 * total / best["copy"] / 1e6, 1),
                              "fill_over_copy": round(best["fill"] / best["copy"], 3), "fill_over_replace_fill": round(best["fill"] / best["replace"], 3),
                              "replace_out_chars": r_total, "pieces_per_16B_block": round(pieces_per_block, 3),
                              "rounds_per_64_block_step": round(rounds_per_step, 3)}), flush=True)
            del out, src, out_len, out_off, text_first, off_first, r_len, r_off, r_out, po, pse
        if wl == "c3":
            words_bits = pattern.contained_in_packed(data, offsets)
            text, off = Pattern.select_rows_packed(data, offsets, words_bits)
            torch.cuda.synchronize()
            total, chosen = int(off[-1].item()), off.numel() - 1
            out = torch.empty((total + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
            src = torch.empty_like(out)
            stages = [("select", lambda: Pattern.select_rows_packed(data, offsets, words_bits, out=out)), ("copy", lambda: out[:total].copy_(src[:total]))]
            for _, fn in stages:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k, _ in stages}
            for _ in range(args.rounds):
                for k, fn in stages:
                    ms[k].append(round(timed(fn), 4))
            best = {k: min(v) for k, v in ms.items()}
            print(json.dumps({"workload": wl, "list": "select", "rows": n, "rows_selected": chosen, "out_chars": total, "ms_per_step": ms, "best_ms": best,
                              "select_over_copy": round(best["select"] / best["copy"], 3)}), flush=True)
            del out, src, text, off
        del data, moff, st, en, lists


if __name__ == "__main__":
    main()
