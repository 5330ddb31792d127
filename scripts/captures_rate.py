#!/usr/bin/env python3
"""Capturing groups: what needle_captures_spans_packed_dev costs beside the closest existing kernel and beside the find-all that feeds
it.  Batch: 10^7 packed 8-bit log-like rows, seeded -- 4096 distinct lines made on the host (a client address, a dash range, a request
line with method, path and HTTP version, a status), drawn at random per row and assembled on the device.  For each of the two patterns
  request   (GET|POST|PUT) (/[^ ]*) HTTP/([0-9])\\.([0-9])
  range     ([0-9]+)-([0-9]+)
the spans are the pattern's own find-all list, and three calls are timed, each step between two HIP events of its own, alternated
step by step in one process after W warm-up steps:
  captures  Pattern.captures_spans_packed on the resident list (captures_spans_kernel, caller-owned planes)
  tags      PatternSet.matches_spans_packed of the one-member set of the same pattern on the same list (set_spans_kernel: the same
            skeleton, one table lookup per char, no tags, one word per span out)
  find_all  Pattern.find_all_packed (count, cumsum, the total read back, fill): what produces the list
Before timing, the planes of a sample of rows are compared with re.  The share of transitions that ran an op list is counted on the
CPU walk of the exported tables over every distinct line's matches, weighted by how often the line was drawn.
python scripts/captures_rate.py [--rows N] [--steps K] [--warmup W] [--md PATH]"""
import argparse
import json
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATTERNS = {"request": r"(GET|POST|PUT) (/[^ ]*) HTTP/([0-9])\.([0-9])", "range": r"([0-9]+)-([0-9]+)"}


def make_lines(count=4096, seed=9):
    rng = random.Random(seed)
    word = lambda a, b: "".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789_") for _ in range(rng.randint(a, b)))
    lines = []
    for _ in range(count):
        ip = ".".join(str(rng.randint(1, 254)) for _ in range(4))
        lo = rng.randint(0, 99999)
        path = "/" + "/".join(word(1, 9) for _ in range(rng.randint(0, 4)))
        method = rng.choice(["GET", "GET", "GET", "POST", "PUT", "HEAD"])
        lines.append('%s bytes %d-%d "%s %s HTTP/%d.%d" %d' % (ip, lo, lo + rng.randint(1, 9999), method, path, rng.randint(1, 2), rng.randint(0, 1),
                                                                 rng.choice([200, 200, 204, 301, 404, 500])))
    return lines


def op_share(tables, cre, lines, weight):
    """(transitions that ran an op list, transitions) over every match of every line, weighted."""
    cmap, nxt, opid = tables["class_map"], tables["next"], tables["op_id"]
    ran = total = 0
    for line, w in zip(lines, weight):
        for m in cre.finditer(line):
            st = tables["start"]
            for ch in m.group(0):
                c = cmap[ord(ch)]
                ran += w * (int(opid[st, c]) != 0)
                total += w
                st = int(nxt[st, c])
    return ran, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from needle_amd.pattern import DFACompiler, PatternSet, pack_bytes
    if not torch.cuda.is_available():
        raise SystemExit("captures_rate.py measures on the GPU: no device here, nothing measured")
    dev = torch.device("cuda", 0)
    n = args.rows
    lines = make_lines()
    tdata, toff = pack_bytes([l.encode("latin-1") for l in lines])
    tdata, toff = torch.from_numpy(np.ascontiguousarray(tdata)).to(dev), torch.from_numpy(np.asarray(toff).astype(np.int64)).to(dev)
    tlen = torch.diff(toff)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2024101)
    pick = torch.randint(0, len(lines), (n,), device=dev, generator=gen)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(tlen[pick], 0)
    chars = int(offsets[-1].item())
    data = torch.zeros((chars + 3) // 4 * 4 + 16, dtype=torch.uint8, device=dev)
    step = 1 << 20
    for r0 in range(0, n, step):  # (a million rows at a time: the index tensors stay small)
        r1 = min(n, r0 + step)
        ln = tlen[pick[r0:r1]]
        src0 = torch.repeat_interleave(toff[pick[r0:r1]] - (offsets[r0:r1] - offsets[r0]), ln)
        k = torch.arange(int(offsets[r1] - offsets[r0]), device=dev)
        data[int(offsets[r0]):int(offsets[r1])] = tdata[src0 + k]
    weight = torch.bincount(pick, minlength=len(lines)).cpu().tolist()
    result = {"rows": n, "chars": chars, "steps": args.steps, "warmup": args.warmup, "patterns": {}}
    for name, regex in PATTERNS.items():
        p, cre = DFACompiler.compile(regex, name), re.compile(regex)
        ps = PatternSet([p])
        off, st, en = p.find_all_packed(data, offsets)
        m = st.numel()
        planes = (torch.empty((p.group_count() + 1, m), dtype=torch.int32, device=dev), torch.empty((p.group_count() + 1, m), dtype=torch.int32, device=dev))
        masks = torch.empty(m, dtype=torch.int32, device=dev)
        p.captures_spans_packed(data, offsets, off, st, en, out=planes)
        torch.cuda.synchronize()
        nr = min(2000, n)
        h_off, h_pick = off[:nr + 1].cpu().numpy(), pick[:nr].cpu().numpy()
        gs, ge = planes[0][:, :int(h_off[-1])].cpu().numpy(), planes[1][:, :int(h_off[-1])].cpu().numpy()
        for r in range(nr):  # the first rows against re
            want = [[mt.span(g) for g in range(cre.groups + 1)] for mt in cre.finditer(lines[int(h_pick[r])])]
            got = [[(int(gs[g, k]), int(ge[g, k])) for g in range(cre.groups + 1)] for k in range(int(h_off[r]), int(h_off[r + 1]))]
            assert got == want, (name, r, got, want)
        calls = {"captures": lambda: p.captures_spans_packed(data, offsets, off, st, en, out=planes),
                 "tags": lambda: ps.matches_spans_packed(data, offsets, off, st, en, out=masks),
                 "find_all": lambda: p.find_all_packed(data, offsets)}
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
        ran, total = op_share(p.captures_tables(), cre, lines, weight)
        info = p.captures_info()
        result["patterns"][name] = {
            "regex": regex, "spans": m, "span_chars": int((en - st).sum().item()), "ms": stat,
            "program": {k: info[k] for k in ("n_groups", "n_states", "n_cols", "max_threads", "n_slots", "n_op_lists", "n_ops", "lds_bytes")},
            "find_all_route": p.find_all_packed_route(1), "spans_per_second": round(m / (stat["captures"]["median_ms"] * 1e-3)),
            "captures_over_tags": round(stat["captures"]["median_ms"] / stat["tags"]["median_ms"], 3),
            "captures_over_find_all": round(stat["captures"]["median_ms"] / stat["find_all"]["median_ms"], 3),
            "op_list_share": round(ran / max(total, 1), 4), "plane_bytes_out": 8 * (p.group_count() + 1) * m}
        del planes, masks, off, st, en
    print(json.dumps(result), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(result))


def markdown(res):
    out = ["# Capturing groups: the capture kernel beside the span-tag kernel and the find-all (scripts/captures_rate.py)", "",
           "%d packed 8-bit log-like rows (%d chars), seeded; %d timed steps after %d warm-up steps, each call between two HIP events of"
           % (res["rows"], res["chars"], res["steps"], res["warmup"]),
           "its own, the three calls alternated step by step in one process.  Times are medians (min .. max) in ms.", ""]
    for name, r in res["patterns"].items():
        pr = r["program"]
        out += ["## `%s`" % r["regex"], "",
                "%d spans, %d chars under them.  Program: %d groups, %d states x %d columns, at most %d threads, %d slots, %d op lists (%d ops), %d bytes"
                % (r["spans"], r["span_chars"], pr["n_groups"], pr["n_states"], pr["n_cols"], pr["max_threads"], pr["n_slots"], pr["n_op_lists"], pr["n_ops"],
                   pr["lds_bytes"]),
                "of LDS.  %.1f %% of the transitions ran an op list.  Find-all route %s." % (100 * r["op_list_share"], r["find_all_route"]), "",
                "| call | median | min | max |", "|---|---|---|---|"]
        for k in ("captures", "tags", "find_all"):
            out.append("| %s | %.4f | %.4f | %.4f |" % (k, r["ms"][k]["median_ms"], r["ms"][k]["min_ms"], r["ms"][k]["max_ms"]))
        out += ["", "captures / tags = %.3f, captures / find_all = %.3f, %.3g spans per second; the planes written are %d bytes (tags: %d)."
                % (r["captures_over_tags"], r["captures_over_find_all"], r["spans_per_second"], r["plane_bytes_out"], 4 * r["spans"]), ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
