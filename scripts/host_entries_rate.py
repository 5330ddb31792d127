"""End-to-end time of the host-buffer entries (needle_*_host: upload, scan, download -- pageable PCIe copies and allocation dominate),
for comparing two builds of the library:

    python scripts/host_entries_rate.py --libs OLD.so NEW.so [--rounds 3] [--seconds 2.5]

Every figure comes from a fresh child process per library (NEEDLE_LIB), the two libraries alternating; a child warms every case up and
then repeats it for `--seconds`, reporting the median.  The spread of OLD's medians over its rounds (A/A) is what a difference has
to exceed to mean anything.  Prints one table; --json FILE keeps every figure."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["matcher_find_us", "find_batch_1Mx64_ms", "find_packed_1M_ragged_ms", "find_packed16_packed_host_ms", "find_all_csr_1Mx64_ms",
         "find_compact_host_ms", "set_contained_in_packed_host_ms"]


def child(seconds, only=None):
    sys.path.insert(0, ROOT)
    import numpy as np
    from needle_amd import workload as W
    from needle_amd.pattern import DFACompiler, PatternSet
    p = DFACompiler.compile("[0-9]+", "d")
    ps = PatternSet([p, DFACompiler.compile("abc|xyz", "a"), DFACompiler.compile("Sherlock", "s")])
    n = 1_000_000
    rows = W.digits_batch(np, 0, n, 64)
    rng = np.random.default_rng(1)
    lens = rng.integers(1, 257, n)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = np.frombuffer(b"abcxyz 0123456789", np.uint8)[rng.integers(0, 17, int(offsets[-1]))]
    text = "see order 66 for details"

    def matcher_loop():
        for _ in range(2000):
            m = p.matcher(text)
            assert m.find()
    work = {
        "matcher_find_us": (matcher_loop, 1e6 / 2000),
        "find_batch_1Mx64_ms": (lambda: p.find_batch(rows), 1e3),
        "find_packed_1M_ragged_ms": (lambda: p.find_packed(data, offsets), 1e3),
        "find_packed16_packed_host_ms": (lambda: p.find_packed16_packed(data, offsets), 1e3),
        "find_all_csr_1Mx64_ms": (lambda: p.find_all_csr(rows), 1e3),
        "find_compact_host_ms": (lambda: p.find_compact(rows), 1e3),
        "set_contained_in_packed_host_ms": (lambda: ps.contained_in_packed(data, offsets), 1e3),
    }
    out = {}
    for name in only or CASES:
        fn, scale = work[name]
        fn()
        fn()
        times, t_end = [], time.perf_counter() + seconds
        while len(times) < 5 or time.perf_counter() < t_end:
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * scale)
        out[name] = {"median": statistics.median(times), "min": min(times), "n": len(times)}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=2.5)
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only", help="--child: comma list of cases (for a run under a tracer)")
    a = ap.parse_args()
    if a.child:
        return child(a.seconds, a.only.split(",") if a.only else None)
    runs = {"old": [], "new": []}
    for _ in range(a.rounds):
        for label, lib in zip(("old", "new"), a.libs):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(a.seconds)], capture_output=True, text=True,
                               env=dict(os.environ, NEEDLE_LIB=os.path.abspath(lib)), timeout=600)
            line = [ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit("child failed (%s, exit %d):\n%s" % (label, r.returncode, (r.stdout + r.stderr)[-3000:]))
            runs[label].append(json.loads(line[0][7:]))
    print("| case | old: median of each round | A/A spread | old median | new: median of each round | new median | new - old | within the spread |")
    print("|---|---|---|---|---|---|---|---|")
    for c in CASES:
        old, new = [r[c]["median"] for r in runs["old"]], [r[c]["median"] for r in runs["new"]]
        spread, mo, mn = max(old) - min(old), statistics.median(old), statistics.median(new)
        fmt = lambda xs: " ".join("%.2f" % x for x in xs)
        print("| %s | %s | %.2f | %.2f | %s | %.2f | %+.2f | %s |" % (c, fmt(old), spread, mo, fmt(new), mn, mn - mo, "yes" if abs(mn - mo) <= spread else "NO"))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
