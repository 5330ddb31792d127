#!/usr/bin/env python3
"""VGPRs / scratch of every instantiation of the tiled scan kernel, of the per-lane and the lock-step find-all kernels of fixed-stride
rows, of the packed-rows scan kernel, of the packed-rows find-all kernels (transducer and per-lane), of the packed-rows pattern-set kernel,
of the pattern-set kernel of span lists (needle_set_spans.h), of the capture kernel of span lists (needle_captures_spans.h) and of the n-gram filter kernels (fixed-stride rows: needle_ngram.hip; packed rows: needle_ngram_packed_*.hip) and of the replace kernels
(needle_replace.hip, needle_replace_each.hip, needle_replace_groups.hip: 4 waves per workgroup, static LDS) and of the gather kernels (needle_gather.hip: the same) and of the UTF-8 kernels (needle_utf8.hip: the same)
and of the line-splitting kernels (needle_lines.hip: one workgroup of 256 lanes per tile, static LDS)
and of the grouping kernels (needle_group.hip: 4 waves per workgroup; the hash kernel's offsets in static LDS)
(cross-compiled here, no
GPU needed): the kernels run 16 waves per workgroup, i.e. at most 128 VGPRs; anything above spills.  The packed-rows kernels'
LDS is the program plus one window (the tile) per wave, sized at launch: listed as the window per wave.
python scripts/kernel_resources.py [--all]"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "needle_amd", "csrc")
names = {"0": "matches", "1": "containedIn", "2": "find"}
modes = {"0": "pack", "1": "table8", "2": "table16", "3": "hbm", "4": "pair", "5": "hot-rows", "6": "sparse"}
procs = []
tmp = tempfile.mkdtemp()
for tu in ("needle_scan_matches", "needle_scan_contained", "needle_scan_find1", "needle_scan_find2",
           "needle_find_all", "needle_find_all_ls",
           "needle_packed_matches", "needle_packed_contained", "needle_packed_find1", "needle_packed_find2", "needle_packed_next1",
           "needle_packed_next2", "needle_packed_forms1", "needle_packed_forms2",
           "needle_packed_find_all1", "needle_packed_find_all2", "needle_packed_find_all_lane1", "needle_packed_find_all_lane2",
           "needle_packed_set1", "needle_packed_set2", "needle_set_spans1", "needle_set_spans2", "needle_captures_spans1", "needle_captures_spans2",
           "needle_ngram", "needle_ngram_packed_contained1", "needle_ngram_packed_contained2", "needle_ngram_packed_find1", "needle_ngram_packed_find2",
           "needle_ngram_packed_find_all1", "needle_ngram_packed_find_all2", "needle_replace", "needle_replace_each", "needle_replace_groups", "needle_gather", "needle_group", "needle_utf8", "needle_lines"):
    out = os.path.join(tmp, tu + ".s")
    procs.append((out, subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only",
                                         "-S", "-o", out, os.path.join(CSRC, tu + ".hip")], stderr=subprocess.DEVNULL)))
rows = []
lds = {}  # static LDS bytes per kernel (the replace kernels' tables; the other kernels size their LDS at launch)
for out, pr in procs:
    pr.wait()
    k = None
    for line in open(out):
        m = re.match(r"\s+\.amdhsa_kernel\s+(\S+)", line)
        if m:
            k = [m.group(1), 0, 0]
            rows.append(k)
        m = re.match(r"\s+\.amdhsa_private_segment_fixed_size\s+(\d+)", line)
        if m and k:
            k[1] = int(m.group(1))
        m = re.match(r"\s+\.amdhsa_group_segment_fixed_size\s+(\d+)", line)
        if m and k:
            lds[k[0]] = int(m.group(1))
        m = re.match(r"\s+\.amdhsa_next_free_vgpr\s+(\d+)", line)
        if m and k:
            k[2] = int(m.group(1))
print("%d kernels; scratch bytes / VGPRs / kernel" % len(rows))
for k, sc, v in sorted(rows):
    m = re.search(r"scan_kernelILi(\d)ELi(\d)ELi(\d)ELb(\d)ELi(\d+)E", k)
    if m and (sc > 0 or "--all" in sys.argv):
        print("%4d %4d  %-11s cw%s %-8s %-5s tile %s" % (sc, v, names[m.group(1)], m.group(2), modes[m.group(3)], "guard" if m.group(4) == "1" else "full", m.group(5)))
# the per-lane find-all kernel of fixed-stride rows is always listed, spilling or not
print("fixed-stride per-lane find-all kernels (needle_find_all.hip): scratch bytes / VGPRs / kernel / tile per lane")
for k, sc, v in sorted(rows):
    m = re.search(r"\d+find_all_kernelILi(\d)ELi(\d)ELi(\d+)ELb(\d)E", k)  # (the digits: the mangled name's length -- not packed_find_all_kernel)
    if m:
        print("%4d %4d  find-all    cw%s %-8s %-11s tile %3d B" % (sc, v, m.group(1), modes[m.group(2)], "skip-states" if m.group(4) == "1" else "", int(m.group(3))))
# ... and so is the lock-step find-all kernel of fixed-stride rows
print("fixed-stride lock-step find-all kernels (needle_find_all_ls.hip): scratch bytes / VGPRs / kernel / tile per lane")
for k, sc, v in sorted(rows):
    m = re.search(r"find_all_lockstep_kernelILi(\d)ELb(\d)ELi(\d+)ELb(\d)E", k)
    if m:
        print("%4d %4d  find-all    cw%s %-8s %-5s tile %3d B" % (sc, v, m.group(1), "run" if m.group(4) == "1" else "lengths", "guard" if m.group(2) == "1" else "full", int(m.group(3))))
# the packed-rows kernels are always listed, spilling or not
print("packed-rows kernels (needle_packed.h): scratch bytes / VGPRs / kernel / LDS window per wave")
for k, sc, v in sorted(rows):
    m = re.search(r"packed_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d+)ELb(\d)ELi(\d)E", k)
    if m:  # (last template argument: the find() variant -- int32 pairs, per-row cursors, one dword / uint16 per row)
        print("%4d %4d  %-11s cw%s %-8s %-7s %-7s window %5d B" % (sc, v, names[m.group(1)], m.group(2), modes[m.group(3)], "lengths" if m.group(5) == "1" else "",
                                                            {"0": "", "1": "cursor", "2": "forms"}[m.group(6)], 64 * int(m.group(4))))
print("packed-rows find-all kernels (needle_packed_find_all.h): scratch bytes / VGPRs / kernel / LDS window per wave")
for k, sc, v in sorted(rows):
    m = re.search(r"packed_find_all_kernelILi(\d)ELi(\d+)ELb(\d)E", k)
    if m:
        print("%4d %4d  find-all    cw%s %-8s window %5d B" % (sc, v, m.group(1), "run" if m.group(3) == "1" else "lengths", 64 * int(m.group(2))))
print("packed-rows per-lane find-all kernels (needle_packed_find_all_lane.h): scratch bytes / VGPRs / kernel / LDS window per wave")
for k, sc, v in sorted(rows):
    m = re.search(r"packed_find_all_lane_kernelILi(\d)ELi(\d)ELi(\d+)ELb(\d)E", k)
    if m:
        print("%4d %4d  find-all    cw%s %-8s %-11s window %5d B" % (sc, v, m.group(1), modes[m.group(2)], "skip-states" if m.group(4) == "1" else "", 64 * int(m.group(3))))
print("packed-rows pattern-set kernels (needle_packed_set.h): scratch bytes / VGPRs / kernel / LDS window per wave")
for k, sc, v in sorted(rows):
    m = re.search(r"packed_set_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d+)E", k)
    if m:
        print("%4d %4d  %-11s cw%s %-8s window %5d B" % (sc, v, names[m.group(1)], m.group(2), modes[m.group(3)], 64 * int(m.group(4))))
# the pattern-set kernel of span lists (needle_set_spans.h): LDS = program + 1040 bytes of offsets per wave, sized at launch
print("pattern-set span kernels (needle_set_spans.h): scratch bytes / VGPRs / kernel / LDS offsets per wave")
for k, sc, v in sorted(rows):
    m = re.search(r"set_spans_kernelILi(\d)ELi(\d)E", k)
    if m:
        print("%4d %4d  span masks  cw%s %-8s offsets %5d B" % (sc, v, m.group(1), modes[m.group(2)], 2 * 65 * 8))
# the capture kernel of span lists (needle_captures_spans.h): LDS = program + per wave 1040 bytes of offsets and 256 bytes per slot, sized at launch
print("capture span kernels (needle_captures_spans.h): scratch bytes / VGPRs / kernel / LDS per wave")
for k, sc, v in sorted(rows):
    m = re.search(r"captures_spans_kernelILi(\d)E", k)
    if m:
        print("%4d %4d  group spans cw%s offsets %5d B + 256 B per slot" % (sc, v, m.group(1), 2 * 65 * 8))
# the n-gram filter kernels (needle_ngram_kernel.h): LDS = program + bitmaps + per wave the queues and slots (packed rows: + the row starts)
names_ng = dict(names, **{"3": "find-all"})
for title, rx in (("n-gram filter kernels, fixed-stride rows (needle_ngram.hip): scratch bytes / VGPRs / kernel", r"ngram_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)E"),
                  ("n-gram filter kernels, packed rows (needle_ngram_packed.h): scratch bytes / VGPRs / kernel", r"ngram_packed_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)ELb(\d)E")):
    print(title)
    for k, sc, v in sorted(rows):
        m = re.search(rx, k)
        if m:
            print("%4d %4d  %-11s %-8s S%s cw%s %s%s" % (sc, v, names_ng[m.group(1)], modes[m.group(2)], m.group(3), m.group(4), "wide " if m.group(5) == "1" else "",
                                                       "backward-walks" if m.lastindex >= 6 and m.group(6) == "1" else ""))
# the replace kernels (needle_replace.hip): the lengths kernel, the fill kernel per char width, the replacement's upload
print("replace kernels (needle_replace.hip): scratch bytes / VGPRs / LDS bytes per workgroup / kernel")
for k, sc, v in sorted(rows):
    m = re.search(r"replace_(lengths|fill|put)_kernel(?:ILi(\d)E)?", k)
    if m:
        print("%4d %4d %6d  replace %-8s %s" % (sc, v, lds.get(k, 0), m.group(1), "cw" + m.group(2) if m.group(2) else ""))
# the replace-each kernels (needle_replace_each.hip): a replacement per match out of a table -- instantiated apart from the plain ones
print("replace-each kernels (needle_replace_each.hip): scratch bytes / VGPRs / LDS bytes per workgroup / kernel")
for k, sc, v in sorted(rows):
    m = re.search(r"replace_each_(lengths|fill)_kernel(?:ILi(\d)E)?", k)
    if m:
        print("%4d %4d %6d  replace-each %-8s %s" % (sc, v, lds.get(k, 0), m.group(1), "cw" + m.group(2) if m.group(2) else ""))
# the replace-groups kernels (needle_replace_groups.hip): a template of literals and group references -- instantiated apart as well
print("replace-groups kernels (needle_replace_groups.hip): scratch bytes / VGPRs / LDS bytes per workgroup / kernel")
for k, sc, v in sorted(rows):
    m = re.search(r"replace_groups_(lengths|fill)_kernel(?:ILi(\d)E)?", k)
    if m:
        print("%4d %4d %6d  replace-groups %-8s %s" % (sc, v, lds.get(k, 0), m.group(1), "cw" + m.group(2) if m.group(2) else ""))
# the gather kernels (needle_gather.hip): span lengths, the split list, the fill kernel per char width
print("gather kernels (needle_gather.hip): scratch bytes / VGPRs / LDS bytes per workgroup / kernel")
for k, sc, v in sorted(rows):
    m = re.search(r"(gather_lengths|split_spans|gather_fill)_kernel(?:ILi(\d)E)?", k)
    if m:
        print("%4d %4d %6d  %-14s %s" % (sc, v, lds.get(k, 0), m.group(1).replace("_", " "), "cw" + m.group(2) if m.group(2) else ""))
# the grouping kernels (needle_group.hip): the hash per char width, insert, finish
print("grouping kernels (needle_group.hip): scratch bytes / VGPRs / LDS bytes per workgroup / kernel")
for k, sc, v in sorted(rows):
    m = re.search(r"group_(hash|insert|finish)_kernel(?:ILi(\d)E)?", k)
    if m:
        print("%4d %4d %6d  group %-6s %s" % (sc, v, lds.get(k, 0), m.group(1), "cw" + m.group(2) if m.group(2) else ""))
# the UTF-8 kernels (needle_utf8.hip): lengths and fill (position-parallel), positions (lane = row)
print("UTF-8 kernels (needle_utf8.hip): scratch bytes / VGPRs / LDS bytes per workgroup / kernel")
for k, sc, v in sorted(rows):
    m = re.search(r"utf8_(lengths|fill|positions)_kernel", k)
    if m:
        print("%4d %4d %6d  utf8 %s" % (sc, v, lds.get(k, 0), m.group(1)))
# the line-splitting kernels (needle_lines.hip): count per char width, fill per char width and mode
print("line-splitting kernels (needle_lines.hip): scratch bytes / VGPRs / LDS bytes per workgroup / kernel")
for k, sc, v in sorted(rows):
    m = re.search(r"lines_(count|fill)_kernelILi(\d)E(?:Lb(\d)E)?", k)
    if m:
        print("%4d %4d %6d  lines %-5s cw%s %s" % (sc, v, lds.get(k, 0), m.group(1), m.group(2), {None: "", "0": "strip", "1": "keep ends"}[m.group(3)]))
