package com.justinblank.strings.gpu;

/**
 * 1 .. 32 compiled patterns answered in ONE pass over a batch of strings (needle_pattern_set, include/needle_hip.h): bit i of a
 * haystack's mask is what {@code patterns[i].matcher(haystack).matches()} / {@code containedIn()} returns.  The reference has no
 * batch API and no sets; a caller with k rules pays one scan per rule without this class, one table lookup per char with it.
 * The patterns' tables are copied at creation: the GpuPattern objects may be closed afterwards.  A pattern whose automaton does
 * not fit the GPU's local memory as a plain table (a dictionary of thousands of keywords) is refused with
 * PatternClassCompilationException naming its index; such patterns run alone.
 *
 * NOT COMPILED IN THE BUILD CONTAINER (no JDK, no jni.h); shipped as source for a maintainer with a JDK.
 */
public final class GpuPatternSet implements AutoCloseable {
    private long handle;
    private final int nPatterns;

    public GpuPatternSet(GpuPattern... patterns) {
        long[] handles = new long[patterns.length];
        for (int i = 0; i < patterns.length; i++) {
            handles[i] = patterns[i].handle();
        }
        long[] out = new long[1];
        GpuPattern.check(Native.setCreate(handles, out), "(pattern set)");
        handle = out[0];
        nPatterns = patterns.length;
    }

    public int size() {
        return nPatterns;
    }

    /** masks[i]: bit j set when pattern j matches() haystacks[i] as a whole. */
    public int[] matchesStrings(String[] haystacks) {
        return run(0, haystacks);
    }

    /** masks[i]: bit j set when pattern j is containedIn() haystacks[i]. */
    public int[] containedInStrings(String[] haystacks) {
        return run(1, haystacks);
    }

    private int[] run(int op, String[] haystacks) {
        long[] offsets = new long[haystacks.length + 1];
        for (int i = 0; i < haystacks.length; i++) {
            offsets[i + 1] = offsets[i] + haystacks[i].length();
        }
        char[] data = new char[(int) offsets[haystacks.length]];
        for (int i = 0; i < haystacks.length; i++) {
            haystacks[i].getChars(0, haystacks[i].length(), data, (int) offsets[i]);
        }
        int[] masks = new int[haystacks.length];
        GpuPattern.check(Native.setPackedHost(handle, op, data, offsets, masks), "(pattern set)");
        return masks;
    }

    /** Result of {@link #tagMatchesStrings}: haystack r's matches are start / end / masks[offsets[r] .. offsets[r + 1]). */
    public static final class TaggedMatches {
        public final long[] offsets;
        public final int[] start;
        public final int[] end;
        /** bit j of masks[m]: pattern j matches() the text of match m as a whole. */
        public final int[] masks;

        TaggedMatches(long[] offsets, int[] start, int[] end, int[] masks) {
            this.offsets = offsets;
            this.start = start;
            this.end = end;
            this.masks = masks;
        }

        /** The lowest set bit of masks[m] -- the convention for "the rule" of a match of a union compiled in member order -- or -1. */
        public int firstMember(int m) {
            return masks[m] == 0 ? -1 : Integer.numberOfTrailingZeros(masks[m]);
        }
    }

    /**
     * Every non-overlapping match of {@code pattern} (typically the union (r0)|(r1)|.. of this set's rules) in every haystack, with the
     * mask of this set's patterns that match it (needle_set_tag_matches_packed_host): a sizing call, then the lists.
     */
    public TaggedMatches tagMatchesStrings(GpuPattern pattern, String[] haystacks) {
        long[] offsets = new long[haystacks.length + 1];
        for (int i = 0; i < haystacks.length; i++) {
            offsets[i + 1] = offsets[i] + haystacks[i].length();
        }
        char[] data = new char[(int) offsets[haystacks.length]];
        for (int i = 0; i < haystacks.length; i++) {
            haystacks[i].getChars(0, haystacks[i].length(), data, (int) offsets[i]);
        }
        long[] matchOffsets = new long[haystacks.length + 1];
        long[] total = new long[1];
        GpuPattern.check(Native.setTagMatchesPackedHost(handle, pattern.handle(), data, offsets, matchOffsets, null, null, null, total), "(pattern set)");
        int[] start = new int[(int) total[0]];
        int[] end = new int[(int) total[0]];
        int[] masks = new int[(int) total[0]];
        if (total[0] > 0) {
            GpuPattern.check(Native.setTagMatchesPackedHost(handle, pattern.handle(), data, offsets, matchOffsets, start, end, masks, total), "(pattern set)");
        }
        return new TaggedMatches(matchOffsets, start, end, masks);
    }

    /**
     * A rule list in one call: every non-overlapping match of {@code pattern} (typically the union (r0)|(r1)|.. of this set's rules) in
     * every haystack is replaced by {@code replacements[j]}, j the LOWEST pattern of this set that matches() the match's text as a
     * whole -- the first rule of an ordered rule list -- and kept as it is when no pattern of the set does.  One replacement per pattern
     * of the set, literal as in {@link GpuPattern#replaceAllStrings}, at most 4096 chars in all; an empty one deletes its rule's
     * matches.  A sizing call, then the call that files the text (needle_set_replace_each_packed_host).
     */
    public String[] replaceEachStrings(GpuPattern pattern, String[] haystacks, String[] replacements) {
        long[] offsets = new long[haystacks.length + 1];
        for (int i = 0; i < haystacks.length; i++) {
            offsets[i + 1] = offsets[i] + haystacks[i].length();
        }
        char[] data = new char[(int) offsets[haystacks.length]];
        for (int i = 0; i < haystacks.length; i++) {
            haystacks[i].getChars(0, haystacks[i].length(), data, (int) offsets[i]);
        }
        int[] replOffsets = new int[replacements.length + 1];
        for (int i = 0; i < replacements.length; i++) {
            replOffsets[i + 1] = replOffsets[i] + replacements[i].length();
        }
        char[] repl = new char[replOffsets[replacements.length]];
        for (int i = 0; i < replacements.length; i++) {
            replacements[i].getChars(0, replacements[i].length(), repl, replOffsets[i]);
        }
        long[] outOffsets = new long[haystacks.length + 1];
        long[] total = new long[1];
        GpuPattern.check(Native.setReplaceEachPackedHost(handle, pattern.handle(), data, offsets, repl, replOffsets, outOffsets, null, total), "(pattern set)");
        if (total[0] > Integer.MAX_VALUE - 8) {
            throw new IllegalArgumentException("the result does not fit a char[]: " + total[0] + " chars");
        }
        char[] out = new char[(int) total[0]];
        if (total[0] > 0) {
            GpuPattern.check(Native.setReplaceEachPackedHost(handle, pattern.handle(), data, offsets, repl, replOffsets, outOffsets, out, total), "(pattern set)");
        }
        String[] result = new String[haystacks.length];
        for (int i = 0; i < haystacks.length; i++) {
            result[i] = new String(out, (int) outOffsets[i], (int) (outOffsets[i + 1] - outOffsets[i]));
        }
        return result;
    }

    /**
     * needle_set_matches_spans_packed_dev for a host whose batch and match list are ALREADY in device memory: every argument but
     * charWidth and nRows is a device address (data 4-byte aligned; offsets and spanOffsets nRows + 1 uint64; start / end int32 relative
     * to the row, 0 only when there are no spans; masks uint32 indexed like start), stream a hipStream_t (0: the null stream).
     * Stream-ordered, nothing is read back; spans are clamped into their rows and need not be sorted.
     */
    public void matchesSpans(long data, int charWidth, long nRows, long offsets, long spanOffsets, long start, long end, long masks, long stream) {
        GpuPattern.check(Native.setMatchesSpansPackedDev(handle, data, charWidth, nRows, offsets, spanOffsets, start, end, masks, stream), "(pattern set)");
    }

    @Override
    public void close() {
        if (handle != 0) {
            Native.setDestroy(handle);
            handle = 0;
        }
    }
}
