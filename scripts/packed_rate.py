#!/usr/bin/env python3
"""Packed device batches: the direct scan (needle_*_packed_dev) against what such a batch cost before.  The rows are bench.py's c2r / c3r
rows (make_pattern / make_rows, per-row lengths (r * 2654435761) % 256 + 1), packed back to back on the device.  Per workload, K steps
between two HIP events after W warm-up steps:
  (a) direct     needle_{contained_in,find}_packed_dev on the packed batch
  (b) convert    needle_rows_from_packed_dev (stride 256, no sync) + the fixed-stride ragged call on its output
  (c) ragged     the fixed-stride ragged call on the 256-byte rows (bench.py's c2r / c3r)
GB/s over ACTUAL bytes: chars + 8 B offset per row + result bytes (bitmap, + 8 B start / end per row for find), fraction of 8 TB/s.
The n-gram filter in front of packed rows (needle_ngram_packed.h): workloads c3sp, c3xp, c3s16p, c3m16p -- bench.py's c3s / c3x / c3s16 /
c3m16 dictionaries and rows with the same lengths, packed -- with the routes alternated inside one process, round by round:
  (a)  the packed call, prefilter AUTO (the filter kernel)
  (a0) the same call after set_prefilter(OFF): the plain packed kernel, i.e. what the call ran before the filter
  (c)  the fixed-stride ragged call on the same rows
and two extras: `long` (rows of 70 000 and 1 MiB chars among 10 000 short ones: (a) against (a0) -- long rows filtered by their group's
whole wave against one lane per row) and `flood` (the flood text of tests/test_gpu_prefilter_watch.py, packed ragged: (a) pinned ON against (a0),
with the candidates per KiB the watch saw).
python scripts/packed_rate.py [--rows N] [--steps K] [--warmup W] [--only c2p,c3p,c3sp,c3xp,c3s16p,c3m16p,long,flood] [--which a,b,c] [--rounds R]"""
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
    ap.add_argument("--rounds", type=int, default=2, help="filter workloads: timed windows per route, alternated a / a0 / c")
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
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def launches(p):
        return p.prefilter_state("forwards")["filter_launches"] + p.prefilter_state("contained_in")["filter_launches"]

    def ab(p, call, routes, rounds):
        """routes: [(tag, prefilter mode or None, fn)] alternated round by round -> {tag: [ms per step of every round]}, launches per tag"""
        out, ran = {t: [] for t, _, _ in routes}, {}
        for t, mode, fn in routes:
            if mode is not None:
                p.set_prefilter(mode)
            for _ in range(max(3, args.warmup)):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for t, mode, fn in routes:
                if mode is not None:
                    p.set_prefilter(mode)
                b = launches(p)
                out[t].append(round(timed(fn), 4))
                ran[t] = launches(p) - b
        p.set_prefilter(p.PREFILTER_AUTO)
        return out, ran

    for wl in args.only.split(","):
        if wl in ("c3sp", "c3xp", "c3s16p", "c3m16p"):
            base = wl[:-1]
            pattern, what, words = bench.make_pattern(base)
            rows = bench.make_rows(base, words, 0, n, dev)
            cw = rows.element_size()
            data = torch.empty(chars, dtype=rows.dtype, device=dev)
            for s in range(0, n, 1 << 20):
                k = min(1 << 20, n - s)
                data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
            bm = torch.empty(words_n, dtype=torch.int64, device=dev)
            st = torch.empty(n, dtype=torch.int32, device=dev)
            en = torch.empty(n, dtype=torch.int32, device=dev)
            sums = {}

            def packed_call():
                pattern.find_packed(data, offsets, out=(bm, st, en))

            def ragged_call():
                pattern.find_batch(rows, l32, out=(bm, st, en))
            for tag, mode, fn in (("a", pattern.PREFILTER_AUTO, packed_call), ("a0", pattern.PREFILTER_OFF, packed_call), ("c", pattern.PREFILTER_AUTO, ragged_call)):
                pattern.set_prefilter(mode)
                fn()
                torch.cuda.synchronize()
                sums[tag] = (int(unpack_bitmap(bm, n).sum()), int(st.to(torch.int64).sum().item()) + int(en.to(torch.int64).sum().item()))
            assert len(set(sums.values())) == 1, sums
            ms, ran = ab(pattern, None, [("a", pattern.PREFILTER_AUTO, packed_call), ("a0", pattern.PREFILTER_OFF, packed_call), ("c", pattern.PREFILTER_AUTO, ragged_call)],
                         args.rounds)
            actual = chars * cw + n * 8 + words_n * 8 + n * 8
            best = {t: min(v) for t, v in ms.items()}
            print(json.dumps({"workload": wl, "what": what + ", per-row lengths uniform in [1, 256], packed", "rows": n, "chars": chars, "actual_bytes": actual,
                              "matched": sums["a"][0], "ms_per_step": ms, "filter_launches_per_window": ran,
                              "GB/s": {t: round(actual / v / 1e6, 1) for t, v in best.items()},
                              "a0_over_a": round(best["a0"] / best["a"], 2), "a_over_c": round(best["a"] / best["c"], 2),
                              "state": pattern.prefilter_state("forwards")}), flush=True)
            del rows, data, bm, st, en
            continue
        if wl in ("long", "flood"):
            import numpy as np
            from needle_amd import workload as W
            pattern, what, words = bench.make_pattern("c3s")
            rng = np.random.default_rng(17 if wl == "long" else 5)
            if wl == "long":
                al = np.array([ord(ch) for ch in "abcdefghijklmnopqrstuvwxyz "], dtype=np.uint8)
                hrows = [rng.choice(al, int(k)).astype(np.uint8) for k in rng.integers(0, 61, 10000)]
                for k, m in enumerate((70000, 1 << 20) * 5):
                    hrows.insert(37 + k * 811, rng.choice(al, m).astype(np.uint8))
            else:
                m, stride = 64 * 200 + 9, 256
                lw = [w for w in words if len(w) >= 6][:512]
                wt8 = np.full((len(lw), 8), 32, dtype=np.uint8)
                for i, w in enumerate(lw):
                    t = np.array([ord(c) for c in w[-8:]], dtype=np.uint8)
                    t[0] = ord("q") if t[0] != ord("q") else ord("z")
                    wt8[i, 8 - t.size:] = t
                flood = wt8[rng.integers(0, len(lw), (m, stride // 8))].reshape(m, stride)
                hl = rng.integers(100, stride + 1, m)
                hrows = [flood[i, :hl[i]] for i in range(m)]
            hoff = np.zeros(len(hrows) + 1, dtype=np.int64)
            hoff[1:] = np.cumsum([r.size for r in hrows])
            d = torch.from_numpy(np.concatenate(hrows)).to(dev)
            o = torch.from_numpy(hoff).to(dev)
            m = len(hrows)
            bm = torch.empty((m + 63) // 64, dtype=torch.int64, device=dev)
            st = torch.empty(m, dtype=torch.int32, device=dev)
            en = torch.empty(m, dtype=torch.int32, device=dev)

            def packed_call():
                pattern.find_packed(d, o, out=(bm, st, en))
            ms, ran = ab(pattern, None, [("a", pattern.PREFILTER_ON, packed_call), ("a0", pattern.PREFILTER_OFF, packed_call)], args.rounds)
            print(json.dumps({"workload": wl, "rows": m, "chars": int(hoff[-1]), "ms_per_step": ms, "filter_launches_per_window": ran,
                              "state": pattern.prefilter_state("forwards")}), flush=True)
            continue
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
