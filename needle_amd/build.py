"""Builds libneedle_hip.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.  `python -m needle_amd.build`"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libneedle_hip.so")
SOURCES = ["needle_scan_find1.hip", "needle_scan_find2.hip", "needle_scan_contained.hip", "needle_scan_matches.hip", "needle_packed_find1.hip",
           "needle_packed_find2.hip", "needle_packed_contained.hip", "needle_packed_matches.hip", "needle_packed_next1.hip", "needle_packed_next2.hip", "needle_packed_forms1.hip", "needle_packed_forms2.hip", "needle_packed_find_all1.hip",
           "needle_packed_find_all2.hip", "needle_packed_find_all_lane1.hip", "needle_packed_find_all_lane2.hip", "needle_packed_set1.hip", "needle_packed_set2.hip", "needle_set_spans1.hip", "needle_set_spans2.hip", "needle_captures_spans1.hip", "needle_captures_spans2.hip", "needle_kernels.hip",
           "needle_stripe.hip", "needle_find_all.hip", "needle_find_all_ls.hip", "needle_compact.hip", "needle_ngram.hip", "needle_ngram_packed_contained1.hip", "needle_ngram_packed_contained2.hip", "needle_ngram_packed_find1.hip",
           "needle_ngram_packed_find2.hip", "needle_ngram_packed_find_all1.hip", "needle_ngram_packed_find_all2.hip", "needle_replace.hip", "needle_replace_each.hip", "needle_replace_groups.hip", "needle_gather.hip", "needle_group.hip", "needle_utf8.hip", "needle_lines.hip", "needle_ngram_host.cpp", "needle_api.cpp", "needle_host.cpp", "needle_tuning.cpp", "needle_multi.cpp", "needle_lower.cpp", "needle_set.cpp", "needle_regex.cpp", "needle_captures.cpp"]


TUNING_LIB = os.path.join(HERE, "libneedle_hip_tuning.so")
TUNING_SOURCES = SOURCES + ["needle_dict.hip"]


PROBE_LIB = os.path.join(HERE, "libneedle_probe.so")  # measurement aid for bench.py, not part of the product ABI
PROBE_SRCS = [os.path.join(CSRC, "stream_probe.hip"), os.path.join(CSRC, "prefix_probe.hip"), os.path.join(CSRC, "ngram_probe.hip")]


def build_probe(force=False):
    """Measurement kernels: the trivial read-reduce kernel bench.py uses to measure this GPU's streaming-read ceiling, and the
    literal-prefix scan behind the f-4 A/B (scripts/prefix_prefilter_ab.py)."""
    if force or not os.path.exists(PROBE_LIB) or any(os.path.getmtime(f) > os.path.getmtime(PROBE_LIB) for f in PROBE_SRCS):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-o", PROBE_LIB] + PROBE_SRCS)
    return PROBE_LIB


def _stale(lib=LIB, sources=SOURCES):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(f) > t for src in sources for f in _deps(os.path.join(CSRC, src)))


def _deps(path, seen=None):
    """`path` and every file it #includes with quotes, transitively (resolved next to the includer, then in include/)."""
    import re
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    with open(path, errors="replace") as f:
        for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', f.read(), flags=re.M):
            for base in (os.path.dirname(path), os.path.join(HERE, "..", "include")):
                cand = os.path.join(base, inc)
                if os.path.exists(cand):
                    _deps(cand, seen)
                    break
    return seen


def build(force=False, verbose=False):
    build_probe(force)
    if not force and not _stale():
        return LIB
    return _build_lib(LIB, SOURCES, os.path.join(HERE, "build"), [], force, verbose)


def build_tuning(force=False, verbose=False):
    """The measurement build (what scripts/build_tuning.sh makes): the same sources with -DNEEDLE_TUNING -- switches that change
    ANSWERS, never in libneedle_hip.so -- plus needle_dict.hip's two-sets-per-wave kernel, as libneedle_hip_tuning.so.  The
    survivor-pool tests run that kernel through it (NEEDLE_LIB)."""
    if not force and not _stale(TUNING_LIB, TUNING_SOURCES):
        return TUNING_LIB
    return _build_lib(TUNING_LIB, TUNING_SOURCES, os.path.join(HERE, "build", "tuning"), ["-DNEEDLE_TUNING"], force, verbose)


def _build_lib(lib, sources, objdir, defines, force, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-x", "hip", "-Wall", "-Wno-unused-variable"] + defines
    os.makedirs(objdir, exist_ok=True)
    procs, objs = [], []
    for src in sources:  # one hipcc per translation unit, all at once (the scan kernel's 96 instantiations dominate)
        obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(f) for f in _deps(os.path.join(CSRC, src))):
            continue  # (the object is newer than its source and every header it includes, transitively)
        cmd = flags + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", lib] + objs
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    return lib


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
