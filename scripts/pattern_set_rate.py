#!/usr/bin/env python3
"""Pattern sets: ONE containedIn() pass of a PatternSet (needle_set_contained_in_packed_dev) against the SUM of the k single-pattern
needle_contained_in_packed_dev calls a caller pays without it.  Batch: scripts/packed_rate.py's lengths ((r * 2654435761) % 256 + 1 chars per
row, 10^7 rows, packed back to back on the device); text: letters of the set's alphabet, seeded, with one of the set's pieces planted in
every 16th row.  The two routes are alternated in one process, round by round, K steps between two HIP events after W warm-up steps; the
best window of each route counts.  Before timing, the set's masks are compared with the k bitmaps on the whole batch.
python scripts/pattern_set_rate.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--only logs8,kw32,mix16]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=300)  # a window of the set route (0.8 .. 1.2 ms a step) lasts a quarter of a second
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="logs8,kw32,mix16")
    args = ap.parse_args()
    import numpy as np
    import torch
    from needle_amd.pattern import DFACompiler, PatternSet
    from pattern_set_cases import SETS
    if not torch.cuda.is_available():
        raise SystemExit("pattern_set_rate.py measures on the GPU: no device here, nothing measured")
    dev = torch.device("cuda", 0)
    n = args.rows
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
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

    for name in args.only.split(","):
        pats, _, alphabet, pieces = SETS[name]
        k = len(pats)
        gen = torch.Generator(device=dev)
        gen.manual_seed(20240 + k)
        alpha = torch.tensor([ord(c) for c in alphabet], dtype=torch.uint8, device=dev)
        data = torch.empty((chars + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        for s in range(0, data.numel(), 1 << 28):
            e = min(data.numel(), s + (1 << 28))
            data[s:e] = alpha[torch.randint(0, alpha.numel(), (e - s,), device=dev, generator=gen)]
        for j, piece in enumerate(pieces):  # one piece in every 16th row that can hold it, 2 chars in
            rows = torch.arange(j, n, 16 * len(pieces), device=dev)
            rows = rows[lens[rows] >= len(piece) + 2]
            for i, ch in enumerate(piece):
                data[offsets[rows] + 2 + i] = ord(ch)
        singles = [DFACompiler.compile(p, "p%d" % i) for i, p in enumerate(pats)]
        ps = PatternSet(singles)
        info = ps.info("contained_in", 1)
        masks = torch.empty(n, dtype=torch.int32, device=dev)
        bms = [torch.empty(words_n, dtype=torch.int64, device=dev) for _ in range(k)]

        def set_call():
            ps.contained_in_packed(data, offsets, out=masks)

        def separate_calls():
            for p, bm in zip(singles, bms):
                p.contained_in_packed(data, offsets, out=bm)
        # the two routes must agree on every row of the batch that is timed
        set_call()
        separate_calls()
        torch.cuda.synchronize()
        shifts = torch.arange(64, device=dev, dtype=torch.int64)
        want = torch.zeros(n, dtype=torch.int64, device=dev)
        per_pattern = []
        for i, bm in enumerate(bms):
            bits = ((bm[:, None] >> shifts[None, :]) & 1).reshape(-1)[:n]
            per_pattern.append(int(bits.sum().item()))
            want |= bits << i
        got = masks.to(torch.int64) & 0xFFFFFFFF
        assert bool((got == want).all().item()), (name, int((got != want).sum().item()))
        del want, got, bits
        ms = {"set": [], "separate": []}
        for fn in (set_call, separate_calls):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            ms["set"].append(round(timed(set_call), 4))
            ms["separate"].append(round(timed(separate_calls), 4))
        best = {t: min(v) for t, v in ms.items()}
        print(json.dumps({"set": name, "patterns": k, "rows": n, "chars": chars, "groups": info["n_groups"],
                          "states": [g["n_states"] for g in info["groups"]], "columns": [g["n_columns"] for g in info["groups"]],
                          "kernel_mode": [g["kernel_mode"] for g in info["groups"]], "lds_bytes": [g["lds_bytes"] for g in info["groups"]],
                          "rows_matched_per_pattern": per_pattern, "ms_per_step": ms, "best_ms": best,
                          "separate_over_set": round(best["separate"] / best["set"], 2),
                          "separate_ms_per_pattern": round(best["separate"] / k, 4)}), flush=True)
        del data, masks, bms, singles, ps


if __name__ == "__main__":
    main()
