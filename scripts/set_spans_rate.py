#!/usr/bin/env python3
"""Tags for a match list: what needle_set_matches_spans_packed_dev costs beside the find-all that feeds it and beside a full read of
the text.  Batch: 10^7 packed 8-bit rows of 225 .. 288 chars (256 on average) over [a-z ], seeded, with 0 .. 2 of the KW32 keywords
(tests/pattern_set_cases.py) planted per row -- the recipe of test_kw32_against_the_single_pattern_scans at this size, built on the
device.  The spans are the find-all of the set's union pattern.  Three calls are timed, each step between two HIP events of its own,
the three alternated step by step in one process after W warm-up steps:
  spans     PatternSet.matches_spans_packed on the resident match list (the new kernel, caller-owned mask tensor)
  find_all  Pattern.find_all_packed of the union pattern (count, cumsum, the total read back, fill): what produces the list
  rows      PatternSet.matches_packed of the whole rows (needle_set_matches_packed_dev): the yardstick of a full read of the text
Per call: median, min and max of the K step times; spans per second from the median.  Before timing, every mask is checked to name
exactly one keyword, and on a sample that keyword is compared with the text under the span.
python scripts/set_spans_rate.py [--rows N] [--steps K] [--warmup W]"""
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
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from needle_amd.pattern import DFACompiler, PatternSet
    from pattern_set_cases import KW32, SETS
    if not torch.cuda.is_available():
        raise SystemExit("set_spans_rate.py measures on the GPU: no device here, nothing measured")
    dev = torch.device("cuda", 0)
    n = args.rows
    gen = torch.Generator(device=dev)
    gen.manual_seed(2024032)
    lens = torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 64 + 225
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    chars = int(offsets[-1].item())
    alpha = torch.tensor([ord(c) for c in SETS["kw32"][2]], dtype=torch.uint8, device=dev)
    data = torch.empty((chars + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    for s in range(0, data.numel(), 1 << 28):
        e = min(data.numel(), s + (1 << 28))
        data[s:e] = alpha[torch.randint(0, alpha.numel(), (e - s,), device=dev, generator=gen)]
    planted = torch.randint(0, 3, (n,), device=dev, generator=gen)  # keywords per row
    for j in range(2):
        rows = torch.nonzero(planted > j).reshape(-1)
        which = torch.randint(0, 32, (rows.numel(),), device=dev, generator=gen)
        frac = torch.rand(rows.numel(), device=dev, generator=gen, dtype=torch.float64)
        for k, w in enumerate(KW32):
            r = rows[which == k]
            at = offsets[r] + (frac[which == k] * (lens[r] - len(w) + 1).to(torch.float64)).to(torch.int64)
            for i, ch in enumerate(w):
                data[at + i] = ord(ch)
    del planted, frac, which, rows

    ps = PatternSet([DFACompiler.compile(w, "w%d" % i) for i, w in enumerate(KW32)])
    union = ps.union_pattern()
    off, st, en = union.find_all_packed(data, offsets)
    m = st.numel()
    masks = torch.empty(m, dtype=torch.int32, device=dev)
    row_masks = torch.empty(n, dtype=torch.int32, device=dev)
    ps.matches_spans_packed(data, offsets, off, st, en, out=masks)
    torch.cuda.synchronize()
    # every span is exactly one keyword; on a sample, the keyword under the span
    got = masks.to(torch.int64) & 0xFFFFFFFF
    assert bool(((got != 0) & ((got & (got - 1)) == 0)).all().item()), "a span's mask does not name exactly one keyword"
    sample = torch.randint(0, m, (20000,), device=dev, generator=gen)
    row_of = torch.searchsorted(off, sample, right=True) - 1
    h_at = (offsets[row_of] + st[sample]).cpu().numpy()
    h_len = (en[sample] - st[sample]).cpu().numpy()
    h_member = ps.first_member(masks[sample])
    for a, l, k in zip(h_at[:2000], h_len[:2000], h_member[:2000]):
        assert bytes(data[int(a):int(a) + int(l)].cpu().numpy()).decode() == KW32[int(k)], (a, l, k)
    del got

    calls = {"spans": lambda: ps.matches_spans_packed(data, offsets, off, st, en, out=masks),
             "find_all": lambda: union.find_all_packed(data, offsets),
             "rows": lambda: ps.matches_packed(data, offsets, out=row_masks)}
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in calls}
    for _ in range(args.steps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in events.items()}
    stat = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)} for k, v in ms.items()}
    per_row = torch.diff(off)
    info = ps.info("matches", 1)["groups"][0]
    print(json.dumps({"rows": n, "chars": chars, "spans": m, "span_chars": int((en - st).sum().item()),
                      "rows_with_3_or_more_spans": int((per_row >= 3).sum().item()), "steps": args.steps, "warmup": args.warmup,
                      "program": {k: info[k] for k in ("n_states", "n_columns", "kernel_mode", "lds_bytes")},
                      "find_all_route": union.find_all_packed_route(1), "ms": stat,
                      "spans_per_second": round(m / (stat["spans"]["median_ms"] * 1e-3)),
                      "spans_over_rows": round(stat["spans"]["median_ms"] / stat["rows"]["median_ms"], 3)}), flush=True)


if __name__ == "__main__":
    main()
