#!/usr/bin/env python3
"""UTF-8 packed rows through the front door (needle_utf16_lengths_from_utf8_packed_dev / needle_utf16_from_utf8_packed_dev /
needle_utf8_positions_packed_dev) beside the find-all they feed, and the fill kernel against a plain device-to-device copy that moves as
many bytes.  10^7 packed rows, per-row lengths (r * 2654435761) % 256 + 1 bytes, two texts:
  ascii  bench.py's c3 rows (make_pattern / make_rows), pure ASCII
  mixed  per character 70 % ASCII, 15 % Cyrillic, 10 % CJK, 4 % astral, 1 % ill-formed bytes, seeded, built on the device; the rows are
         cut from one stream of characters, so a row's end may cut a sequence (ill-formed by the rule: a little above the 1 %)
The pattern is c3's 1000-keyword union on both (the mixed text has few matches: its list is short).
Stages, each between two HIP events, K steps a window, the stages ALTERNATED in one process, R windows each, the best one counts:
  lengths    needle_utf16_lengths_from_utf8_packed_dev (with both bitmaps)
  cumsum     torch.cumsum of the lengths
  fill       needle_utf16_from_utf8_packed_dev
  copy       dst.copy_(src) of (N + 2 U) / 2 bytes: as many bytes read + written as fill's N read, 2 U written -- the yardstick
  find_all   count, cumsum, CSR fill on the UTF-16 batch already resident: the route without this front door
  positions  needle_utf8_positions_packed_dev on the match list's start array
  chain      lengths, cumsum, fill, find_all, positions on start and on end
Before timing: 2000 sampled rows' units and positions against tests/utf8_cases.py, and (--check-all) every row's length against
CPython's decoder, which tests/test_utf8_abi.py pins the rule to.
python scripts/utf8_rate.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--only ascii,mixed] [--check-all]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def mixed_text(n_bytes, dev, seed=1, slab=1 << 25):
    """At least n_bytes of seeded mixed text on the device, slab by slab."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    probs = torch.tensor([0.70, 0.15, 0.10, 0.04, 0.01], device=dev)
    k_len = torch.tensor([1, 2, 3, 4, 1], device=dev)
    lo = torch.tensor([0x20, 0x430, 0x4E00, 0x1F600, 0], device=dev)
    span = torch.tensor([0x5F, 0x20, 0x1000, 0x50, 1], device=dev)
    ill = torch.tensor([0x80, 0xBF, 0xC0, 0xE2, 0xF0, 0xF5, 0xFF, 0xED], device=dev)
    parts, have = [], 0
    while have < n_bytes:
        n = slab
        kind = torch.multinomial(probs, n, replacement=True, generator=g)
        cp = lo[kind] + (torch.rand(n, device=dev, generator=g) * span[kind]).long()
        k = k_len[kind]
        at = torch.cumsum(k, 0) - k
        out = torch.zeros(int((at[-1] + k[-1]).item()), dtype=torch.uint8, device=dev)
        lead = torch.where(kind == 4, ill[at % 8],
                           torch.where(k == 1, cp, torch.where(k == 2, 0xC0 | (cp >> 6), torch.where(k == 3, 0xE0 | (cp >> 12), 0xF0 | (cp >> 18)))))
        out[at] = lead.to(torch.uint8)
        for j in (1, 2, 3):  # continuation byte j of the sequences that have one
            m = k > j
            out[at[m] + j] = (0x80 | ((cp[m] >> (6 * (k[m] - 1 - j))) & 0x3F)).to(torch.uint8)
        parts.append(out)
        have += out.numel()
    return torch.cat(parts)[:(n_bytes + 3) // 4 * 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="ascii,mixed")
    ap.add_argument("--check-all", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import utf8_cases as U
    from needle_amd import _lib
    from needle_amd.pattern import Pattern
    if not torch.cuda.is_available():
        raise SystemExit("utf8_rate.py measures on the GPU: no device here, nothing measured")
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = args.rows
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    N = int(offsets[-1].item())
    stream = torch.cuda.current_stream(dev).cuda_stream
    pattern, what, words = bench.make_pattern("c3")
    h = pattern._h

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

    for text in args.only.split(","):
        if text == "ascii":
            rows = bench.make_rows("c3", words, 0, n, dev)
            col = torch.arange(256, device=dev)[None, :]
            data = torch.empty((N + 3) // 4 * 4, dtype=torch.uint8, device=dev)
            for s in range(0, n, 1 << 20):  # packed slab by slab
                k = min(1 << 20, n - s)
                data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
            del rows
        else:
            data = mixed_text(N, dev)
        # a first run through the public composition: the totals, and the buffers every timed step reuses
        units, uoff_first, na, mal = Pattern.utf16_from_utf8_packed(data, offsets)
        moff_first, bs_first, be_first = pattern.find_all_utf8_packed(data, offsets)
        torch.cuda.synchronize()
        Utot, m = int(uoff_first[-1].item()), int(moff_first[-1].item())
        # ---- the answers, before any timing
        host, hoff, hu, huoff = data.cpu().numpy(), offsets.cpu().numpy(), units.cpu().numpy().view(np.uint16), uoff_first.cpu().numpy()
        sample = list(range(0, n, max(1, n // 2000)))[:2000]
        lo_, pos_, ans_ = [0], [], []
        for r in sample:
            row = host[hoff[r]:hoff[r + 1]].tobytes()
            want, _ = U.utf8_units(row)
            assert hu[huoff[r]:huoff[r + 1]].tolist() == want, (text, "units of row", r)
            bm = U.unit_bytes(row)
            pos_ += list(range(len(bm))) + [len(bm) + 4, -1]
            ans_ += bm + [len(row), -1]
            lo_.append(len(pos_))
        sdata = torch.from_numpy(np.concatenate([host[hoff[r]:hoff[r + 1]] for r in sample] + [np.zeros(8, np.uint8)])).to(dev)
        soff = torch.from_numpy(np.cumsum([0] + [int(hoff[r + 1] - hoff[r]) for r in sample])).to(dev)
        got = Pattern.utf8_positions_packed(sdata, soff, torch.tensor(lo_, device=dev), torch.tensor(pos_, dtype=torch.int32, device=dev))
        assert got.cpu().tolist() == ans_, (text, "positions of the sampled rows")
        if args.check_all:
            blob, hl = host.tobytes(), np.diff(huoff)
            for r in range(n):
                assert len(blob[hoff[r]:hoff[r + 1]].decode("utf-8", "replace").encode("utf-16-le", "surrogatepass")) == 2 * hl[r], (text, "length of row", r)
            del blob
        del host, hu
        # ---- stages
        pv = _lib.PackedView()
        pv.data, pv.char_width, pv.n_rows, pv.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
        ulen = torch.empty(n, dtype=torch.int64, device=dev)
        uoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        words_na, words_mal = torch.empty_like(na), torch.empty_like(mal)
        u16 = torch.empty(Utot + 4, dtype=torch.int16, device=dev)
        half = (N + 2 * Utot) // 2
        src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        uv = _lib.PackedView()
        uv.data, uv.char_width, uv.n_rows, uv.offsets = u16.data_ptr(), 2, n, uoff.data_ptr()
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        moff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        st, en = torch.empty(max(m, 1), dtype=torch.int32, device=dev), torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        bs, be = torch.empty_like(st), torch.empty_like(en)

        def f_lengths():
            check(L.needle_utf16_lengths_from_utf8_packed_dev(ctypes.byref(pv), ulen.data_ptr(), words_na.data_ptr(), words_mal.data_ptr(), stream))

        def f_cumsum():
            torch.cumsum(ulen, 0, out=uoff[1:])

        def f_fill():
            check(L.needle_utf16_from_utf8_packed_dev(ctypes.byref(pv), uoff.data_ptr(), u16.data_ptr(), stream))

        def f_copy():
            dst.copy_(src)

        def f_find_all():
            check(L.needle_count_matches_packed_dev(h, ctypes.byref(uv), counts.data_ptr(), stream))
            torch.cumsum(counts, 0, out=moff[1:])
            check(L.needle_find_all_csr_packed_dev(h, ctypes.byref(uv), moff.data_ptr(), st.data_ptr(), en.data_ptr(), None, stream))

        def f_positions():
            check(L.needle_utf8_positions_packed_dev(ctypes.byref(pv), moff.data_ptr(), st.data_ptr(), bs.data_ptr(), stream))

        def f_chain():
            f_lengths()
            f_cumsum()
            f_fill()
            f_find_all()
            f_positions()
            check(L.needle_utf8_positions_packed_dev(ctypes.byref(pv), moff.data_ptr(), en.data_ptr(), be.data_ptr(), stream))

        f_chain()
        torch.cuda.synchronize()
        assert torch.equal(uoff, uoff_first) and torch.equal(u16[:Utot], units) and torch.equal(words_mal, mal) and torch.equal(words_na, na)
        assert torch.equal(moff, moff_first) and torch.equal(bs[:m], bs_first) and torch.equal(be[:m], be_first)
        stages = [("lengths", f_lengths), ("cumsum", f_cumsum), ("fill", f_fill), ("copy", f_copy), ("find_all", f_find_all),
                  ("positions", f_positions), ("chain", f_chain)]
        for _, fn in stages:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in stages}
        for _ in range(args.rounds):
            for name, fn in stages:
                ms[name].append(round(timed(fn), 4))
        best = {k: min(v) for k, v in ms.items()}
        ingest = best["chain"] - best["find_all"]
        print(json.dumps({"text": text, "pattern": what, "rows": n, "bytes": N, "units": Utot, "matches": m,
                          "non_ascii_rows": int(sum(bin(int(w) & (2 ** 64 - 1)).count("1") for w in na.cpu().tolist())),
                          "malformed_rows": int(sum(bin(int(w) & (2 ** 64 - 1)).count("1") for w in mal.cpu().tolist())),
                          "ms_per_step": ms, "best_ms": best,
                          "lengths_GB/s_read": round(N / best["lengths"] / 1e6, 1),
                          "fill_GB/s_read_plus_written": round((N + 2 * Utot) / best["fill"] / 1e6, 1),
                          "copy_GB/s_read_plus_written": round(2 * half / best["copy"] / 1e6, 1),
                          "fill_over_copy": round(best["fill"] / best["copy"], 3),
                          "ingest_ms_chain_minus_find_all": round(ingest, 4), "ingest_share_of_chain": round(ingest / best["chain"], 3),
                          "chain_over_find_all": round(best["chain"] / best["find_all"], 3)}), flush=True)
        del data, units, u16, src, dst, st, en, bs, be, counts, moff, ulen, uoff


if __name__ == "__main__":
    main()
