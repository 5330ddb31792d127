#!/usr/bin/env python3
"""Template replacement: what needle_replace_groups_lengths_packed_dev / needle_replace_groups_fill_packed_dev cost beside the find-all
and the captures passes that feed them, and what the two-source sweep costs beside the plain fill kernel.  Batch: captures_rate.py's --
10^7 packed 8-bit log-like rows, seeded.  Per pattern and template
  request   (GET|POST|PUT) (/[^ ]*) HTTP/([0-9])\\.([0-9])   ->  $2 [$1]
  range     ([0-9]+)-([0-9]+)                                ->  $2-$1
the list is the pattern's own find-all list, the planes its captures, and each call is timed between two HIP events of its own, the
calls alternated step by step in one process after W warm-up steps:
  find_all  Pattern.find_all_packed (count, cumsum, the total read back, fill)
  captures  Pattern.captures_spans_packed on the resident list
  lengths   needle_replace_groups_lengths_packed_dev         fill   needle_replace_groups_fill_packed_dev (offsets resident)
and on the same list a literal-only template (`#`, K = 0) through the new fill kernel beside needle_replace_all_fill_packed_dev with the
same literal (the plain kernel, same output bytes) and beside dst.copy_(src) of those output bytes.
Before timing, the results of the first rows are compared with re.sub.
python scripts/replace_groups_rate.py [--rows N] [--steps K] [--warmup W] [--md PATH]"""
import argparse
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from captures_rate import PATTERNS, make_lines  # noqa: E402

TEMPLATES = {"request": "$2 [$1]", "range": "$2-$1"}
PYTHON_REPL = {"request": r"\2 [\1]", "range": r"\2-\1"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from needle_amd import _lib
    from needle_amd.pattern import DFACompiler, Pattern, _check, pack_bytes
    if not torch.cuda.is_available():
        raise SystemExit("replace_groups_rate.py measures on the GPU: no device here, nothing measured")
    L = _lib.lib()
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
    del src0, k
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
    s = torch.cuda.current_stream(dev).cuda_stream
    result = {"rows": n, "chars": chars, "steps": args.steps, "warmup": args.warmup, "patterns": {}}
    for name, regex in PATTERNS.items():
        p, cre = DFACompiler.compile(regex, name), re.compile(regex)
        off, st, en = p.find_all_packed(data, offsets)
        m, planes_n = st.numel(), p.group_count() + 1
        planes = (torch.empty((planes_n, m), dtype=torch.int32, device=dev), torch.empty((planes_n, m), dtype=torch.int32, device=dev))
        p.captures_spans_packed(data, offsets, off, st, en, out=planes)
        groups, literals = p.parse_template(TEMPLATES[name])
        tm, keep = Pattern._template(groups, literals, 1, planes_n)
        lit, keep_lit = Pattern._template([], ["#"], 1, planes_n)
        hash_ = np.frombuffer(b"#", np.uint8)

        def offsets_of(lens):
            o = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            o[1:] = torch.cumsum(lens, 0)
            return o, torch.empty(int(o[-1].item()) + 16, dtype=torch.uint8, device=dev)
        lens = torch.empty(n, dtype=torch.int64, device=dev)
        lengths = lambda t=tm: _check(L.needle_replace_groups_lengths_packed_dev(ctypes.byref(v), off.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(), m,
                                                                                 planes_n, ctypes.byref(t), lens.data_ptr(), s))
        lengths()
        out_off, out = offsets_of(lens)
        lengths(lit)
        lit_off, lit_out = offsets_of(lens)
        plain_out, copy_dst = torch.empty_like(lit_out), torch.empty_like(lit_out)
        fill = lambda t=tm, oo=out_off, o=out: _check(L.needle_replace_groups_fill_packed_dev(ctypes.byref(v), off.data_ptr(), planes[0].data_ptr(),
                                                                                              planes[1].data_ptr(), m, planes_n, ctypes.byref(t), oo.data_ptr(), o.data_ptr(), s))
        plain = lambda: _check(L.needle_replace_all_fill_packed_dev(ctypes.byref(v), off.data_ptr(), st.data_ptr(), en.data_ptr(), hash_.ctypes.data, 1,
                                                                    lit_off.data_ptr(), plain_out.data_ptr(), s))
        fill()
        fill(lit, lit_off, lit_out)
        plain()
        torch.cuda.synchronize()
        assert torch.equal(lit_out[:int(lit_off[-1])], plain_out[:int(lit_off[-1])]), "the literal-only template against the plain kernel"
        nr = min(2000, n)
        h_off, h_pick, h_out = out_off[:nr + 1].cpu().numpy(), pick[:nr].cpu().numpy(), out[:int(out_off[nr])].cpu().numpy()
        for r in range(nr):  # the first rows against re.sub
            want = cre.sub(PYTHON_REPL[name], lines[int(h_pick[r])]).encode("latin-1")
            assert h_out[h_off[r]:h_off[r + 1]].tobytes() == want, (name, r)
        calls = {"find_all": lambda: p.find_all_packed(data, offsets),
                 "captures": lambda: p.captures_spans_packed(data, offsets, off, st, en, out=planes),
                 "lengths": lengths, "fill": fill,
                 "fill_literal_only": lambda: fill(lit, lit_off, lit_out), "plain_fill": plain, "copy": lambda: copy_dst.copy_(lit_out)}
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
        ms = {k: np.array([a.elapsed_time(b) for a, b in e]) for k, e in events.items()}
        stat = {k: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4)} for k, x in ms.items()}
        med = lambda k: stat[k]["median_ms"]
        result["patterns"][name] = {
            "regex": regex, "template": TEMPLATES[name], "matches": m, "out_bytes": int(out_off[-1].item()), "literal_out_bytes": int(lit_off[-1].item()),
            "pieces_per_match": 1 + len(groups) + sum(1 for x in literals if x), "ms": stat,
            "fill_bytes_per_second": round((chars + int(out_off[-1].item())) / (med("fill") * 1e-3)),
            "fill_over_copy": round(med("fill") / med("copy"), 3), "literal_only_over_plain": round(med("fill_literal_only") / med("plain_fill"), 3),
            "plain_over_copy": round(med("plain_fill") / med("copy"), 3)}
        del planes, off, st, en, out, lit_out, plain_out, copy_dst, keep, keep_lit
    print(json.dumps(result), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(result))


def markdown(res):
    out = ["# Template replacement: the two-source sweep beside its feeders and beside the plain fill (scripts/replace_groups_rate.py)", "",
           "%d packed 8-bit log-like rows (%d chars), seeded; %d timed steps after %d warm-up steps, each call between two HIP events of"
           % (res["rows"], res["chars"], res["steps"], res["warmup"]),
           "its own, the calls alternated step by step in one process.  Times are medians (min .. max) in ms.", ""]
    for name, r in res["patterns"].items():
        out += ["## `%s` -> `%s`" % (r["regex"], r["template"]), "",
                "%d matches, %d pieces a match; the result is %d bytes (literal-only `#`: %d bytes)." % (r["matches"], r["pieces_per_match"], r["out_bytes"],
                                                                                                        r["literal_out_bytes"]), "",
                "| call | median | min | max |", "|---|---|---|---|"]
        for k in ("find_all", "captures", "lengths", "fill", "fill_literal_only", "plain_fill", "copy"):
            out.append("| %s | %.4f | %.4f | %.4f |" % (k, r["ms"][k]["median_ms"], r["ms"][k]["min_ms"], r["ms"][k]["max_ms"]))
        out += ["", "fill: %.3g bytes read and written per second, %.2fx the copy of the literal-only output; literal-only template / plain kernel = %.3f "
                "(plain kernel / copy = %.2f)." % (r["fill_bytes_per_second"], r["fill_over_copy"], r["literal_only_over_plain"], r["plain_over_copy"]), ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
