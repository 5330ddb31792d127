package com.justinblank.strings.gpu;

/**
 * JNI surface of libneedle_hip.so (include/needle_hip.h).  One-to-one with the C ABI; every method returns the
 * library's status code except where noted, and the shim (bindings/jni/needle_jni.c) never throws -- exceptions
 * are raised on the Java side from the status (see GpuPattern.check).
 *
 * The shim is compiled and exercised against a stand-in jni.h and a fake JNIEnv (tests/jni/, tests/test_jni_shim.py,
 * tests/test_gpu_jni_shim.py), and every declaration below is checked against its C definition there (name, return
 * type, parameter list) -- a signature check: this file itself has never been compiled (no JDK in the build image) and
 * the shim has never been loaded by a JVM.  No native is overloaded, so each has the short JNI symbol name.
 * An array argument is required unless its description says it may be null; a required array that is null or shorter
 * than described gives NEEDLE_ERR_INVALID.
 */
final class Native {
    static {
        System.loadLibrary("needle_jni"); // links libneedle_hip.so
    }

    private Native() {
    }

    static native String lastError();

    static native int deviceCount();

    /** needle_compile: regex as UTF-16 code units (String.toCharArray()). handleOut[0] receives the pattern handle. */
    static native int compile(char[] regex, int flags, long[] handleOut);

    /**
     * needle_pattern_from_tables: what DFATableEmitter extracted from needle's own four DFAs.
     * classMap: 65536 bytes (BYTE_CLASSES[0..65535]); tables[i]: flat short[nStates[i] * stride], -1 = none;
     * accepting[i]: byte[nStates[i]]; order of i: matches, containedIn, forwards, backwards.
     */
    static native int fromTables(byte[] classMap, int stride, int[] nStates, int[] maxChar, short[][] tables,
                                 byte[][] accepting, int fixedLen, long[] handleOut);

    static native void destroyPattern(long handle);

    /**
     * Host-buffer batches.  rows: direct ByteBuffer of nRows * rowStride chars (charWidth 1 or 2, native order);
     * lengths: direct buffer of nRows ints or null; bitmap: long[(nRows + 63) / 64]; start/end: int[nRows].
     */
    static native int matchesHost(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows, long rowStride,
                                  int rowLen, java.nio.ByteBuffer lengths, long[] bitmap);

    static native int containedInHost(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows,
                                      long rowStride, int rowLen, java.nio.ByteBuffer lengths, long[] bitmap);

    static native int findHost(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows, long rowStride,
                               int rowLen, java.nio.ByteBuffer lengths, long[] bitmap, int[] start, int[] end);

    /**
     * Packed host batches (needle_*_packed_host): the UTF-16 code units of all haystacks back to back + offsets[n + 1]
     * (what a String[] flattens to).  op: 0 matches, 1 containedIn, 2 find (start/end may be null otherwise).
     */
    static native int packedHost(long handle, int op, char[] data, long[] offsets, long[] bitmap, int[] start, int[] end);

    /**
     * needle_find_all_csr_packed_host: every non-overlapping match of every packed haystack (UTF-16 code units back to back +
     * offsets[n + 1]); matchOffsets long[n + 1]; start / end int[capacity] (null: count only); total long[1].
     */
    static native int findAllPackedHost(long handle, char[] data, long[] offsets, long[] matchOffsets, int[] start, int[] end, long[] total);

    /**
     * needle_find_all_csr_utf8_packed_host / needle_contained_in_utf8_packed_host: packed haystacks of UTF-8 bytes (data byte[] back to
     * back + offsets[n + 1]), decoded on the device as {@code new String(bytes, UTF_8)} decodes them.  start / end are BYTE offsets into
     * the haystack; malformed long[(n + 63) / 64] (may be null): the haystacks that hold ill-formed UTF-8.
     */
    static native int findAllUtf8PackedHost(long handle, byte[] data, long[] offsets, long[] matchOffsets, int[] start, int[] end, long[] total, long[] malformed);

    static native int containedInUtf8PackedHost(long handle, byte[] data, long[] offsets, long[] bitmap, long[] malformed);

    /**
     * needle_replace_all_packed_host: every non-overlapping match of every packed haystack (data + offsets as packedHost) replaced by the
     * literal replacement (UTF-16 code units, at most 4096; empty: the matches are deleted).  outOffsets long[n + 1] and total long[1]
     * are always filled; out char[capacity] (null: size only) holds the result text when total[0] <= capacity.
     */
    static native int replaceAllPackedHost(long handle, char[] data, long[] offsets, char[] replacement, long[] outOffsets, char[] out, long[] total);

    /**
     * needle_gather_matches_packed_host: every non-overlapping match of every packed haystack (mode 0) or every piece between the matches
     * (mode 1) as a row of a new packed batch.  spanOffsets long[n + 1] (haystack i gave the output rows spanOffsets[i] ..
     * spanOffsets[i + 1]) and totals long[2] (output rows, chars) are always filled; outOffsets long[rows + 1] and out char[chars]
     * (null: size only) hold the result when both totals fit.
     */
    static native int gatherMatchesPackedHost(long handle, char[] data, long[] offsets, int mode, long[] spanOffsets, long[] outOffsets, char[] out, long[] totals);

    /**
     * needle_find_packed16_packed_host / needle_find_packed8_packed_host: find() of every packed haystack with a row's result as
     * one int (start | end << 16; haystacks of at most 65 534 chars) or one short (start | (end - start) << 8, 0xFFFF no match,
     * 0xFFFE the match (0, 256); haystacks of at most 256 chars).  Longer haystacks: NEEDLE_ERR_UNSUPPORTED.
     */
    static native int findPacked16PackedHost(long handle, char[] data, long[] offsets, long[] bitmap, int[] startEnd);

    static native int findPacked8PackedHost(long handle, char[] data, long[] offsets, long[] bitmap, short[] startLen);

    /**
     * Pattern sets (needle_pattern_set_*): 1 .. 32 patterns answered in one pass over a packed batch.  setCreate copies the patterns'
     * tables (the patterns may be closed afterwards); setPackedHost: op 0 matches, 1 containedIn; data + offsets as packedHost;
     * masks int[n]: bit i of masks[r] = what pattern i answers for haystack r.
     */
    static native int setCreate(long[] patterns, long[] handleOut);

    static native void setDestroy(long set);

    static native int setPackedHost(long set, int op, char[] data, long[] offsets, int[] masks);

    /**
     * needle_set_tag_matches_packed_host: findAllPackedHost of `pattern` with the set's mask of every match beside it; masks
     * int[capacity] (start / end / masks null: count only).
     */
    static native int setTagMatchesPackedHost(long set, long pattern, char[] data, long[] offsets, long[] matchOffsets, int[] start, int[] end,
                                              int[] masks, long[] total);

    /**
     * needle_set_replace_each_packed_host: replaceAllPackedHost with a replacement per pattern of the set -- replacements char[] back
     * to back (may be empty, not null), replOffsets int[nPatterns + 1]; out char[capacity] (may be null: size only); total long[1].
     */
    static native int setReplaceEachPackedHost(long set, long pattern, char[] data, long[] offsets, char[] replacements, int[] replOffsets,
                                               long[] outOffsets, char[] out, long[] total);

    /** needle_set_matches_spans_packed_dev: every long but nRows is a device address (stream: a hipStream_t). */
    static native int setMatchesSpansPackedDev(long set, long data, int charWidth, long nRows, long offsets, long spanOffsets, long start,
                                               long end, long masks, long stream);

    /** needle_find_all_host: counts int[nRows]; start / end int[nRows * maxPerRow]; more int[1]. */
    static native int findAllHost(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows, long rowStride, int rowLen,
                                  java.nio.ByteBuffer lengths, int maxPerRow, int[] counts, int[] start, int[] end, int[] more);

    /** needle_find_all_packed16_host: counts int[nRows]; startEnd int[nRows * maxPerRow], each match start | end << 16. */
    static native int findAllPacked16Host(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows, long rowStride, int rowLen,
                                          java.nio.ByteBuffer lengths, int maxPerRow, int[] counts, int[] startEnd, int[] more);

    /** needle_find_all_csr_host: offsets long[nRows + 1]; start / end int[capacity] (null: count only); total long[1]. */
    static native int findAllCsrHost(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows, long rowStride, int rowLen,
                                     java.nio.ByteBuffer lengths, long[] offsets, int[] start, int[] end, long[] total);

    /**
     * needle_find_compact_host: find() with the MATCHED rows only, in row order -- records[2 * k] = row, records[2 * k + 1] =
     * start | end << 16 (needle_match_rec as two ints); nMatched long[1] = the number of matched rows (may exceed the room).
     */
    static native int findCompactHost(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows, long rowStride, int rowLen,
                                      java.nio.ByteBuffer lengths, long[] bitmap, int[] records, long[] nMatched);

    /**
     * needle_find_packed16_host: find() with start / end of every row as ONE int, start | end << 16 (0xFFFFFFFF = no match; rows of
     * at most 65 534 chars): the scan kernel stores that form itself, 4 result bytes per row on the device and over PCIe.
     */
    static native int findPacked16Host(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows, long rowStride, int rowLen,
                                       java.nio.ByteBuffer lengths, long[] bitmap, int[] startEnd);

    /**
     * needle_find_packed8_host (round 6): rows of at most 256 chars, ONE short per row -- start | (end - start) << 8; 0xFFFF = no match,
     * 0xFFFE = the match (0, 256): 2 result bytes per row over PCIe.
     */
    static native int findPacked8Host(long handle, java.nio.ByteBuffer rows, int charWidth, long nRows, long rowStride, int rowLen,
                                      java.nio.ByteBuffer lengths, long[] bitmap, short[] startLen);

    /** needle_tuning_info: the library's NEEDLE_* environment switches, tab-separated lines (name, default, current, scope, effect). */
    static native String tuningInfo();

    /** needle_trim_scratch: hand the library's free scratch memory beyond keepBytes back to the driver. */
    static native int trimScratch(long keepBytes);

    /**
     * needle_pattern_prefilter_info: whether containedIn (which = 1) / find (which = 2) of this pattern run behind the n-gram
     * candidate filter on batches of 8-bit rows -- info[0] on, [1] kernel mode, [2] stride, [3] run-up, [4] shortest match,
     * [5] windows, [6] bitmap bytes; returns the reason when there is no filter ("" otherwise).
     */
    static native String prefilterInfo(long handle, int which, int[] info);

    /** needle_pattern_set_prefilter: 0 auto (the flood watch decides), 1 on (never suspended), 2 off (the ordinary kernels). */
    static native int setPrefilter(long handle, int mode);

    /**
     * needle_pattern_prefilter_state (which: 1 containedIn, 2 find): state[0..3] = mode, has_filter, suspended calls left, backoff;
     * rate[0] = candidates per KiB of the last evaluation; counts[0..1] = filter launches, suspended calls.
     */
    static native int prefilterState(long handle, int which, int[] state, float[] rate, long[] counts);

    /**
     * needle_pattern_find_all_packed_filter (charWidth 1 or 2, countOnly 0 or 1): out[0] = 1 when the packed find-all entries take the
     * n-gram filter kernel for this pattern (neither the transducer nor the per-lane kernel takes it and a filter program exists).
     */
    static native int findAllPackedFilter(long handle, int charWidth, int countOnly, int[] out);

    /** needle_pattern_utf16_route: out[0] = the pattern's one page of the BMP (-1: it spans several), out[1] = the substitute byte. */
    static native int utf16Route(long handle, int[] out);

    /** needle_pattern_serialize / needle_pattern_deserialize: the precompiled-pattern blob (Precompile's analogue). */
    static native byte[] serialize(long handle);

    static native int deserialize(byte[] blob, long[] handleOut);

    /**
     * Row sharding over several GPUs of one node from this JVM (needle_multi_*): devices[0] is the root the results are
     * gathered to (one group of RCCL send / receive pairs over xGMI).  scanHostMulti splits a host batch into contiguous
     * row blocks on 64-row boundaries, one per device; op: 0 matches, 1 containedIn, 2 find.
     */
    static native int multiCreate(int[] devices, int flags, long[] handleOut);

    static native void multiDestroy(long multi);

    static native int scanHostMulti(long multi, long pattern, int op, java.nio.ByteBuffer rows, int charWidth, long nRows,
                                    long rowStride, int rowLen, java.nio.ByteBuffer lengths, long[] bitmap, int[] start, int[] end);

    // one Matcher (reference cursor semantics)
    static native int matcherCreate(long pattern, char[] s, long[] handleOut);

    static native void matcherDestroy(long matcher);

    static native int matcherMatches(long matcher, int[] result);

    static native int matcherContainedIn(long matcher, int[] result);

    static native int matcherFind(long matcher, int[] result);

    static native int matcherFindRange(long matcher, int from, int to, int[] result);

    static native int matcherStart(long matcher);

    static native int matcherEnd(long matcher);
}
