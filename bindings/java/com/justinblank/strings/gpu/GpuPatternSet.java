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

    @Override
    public void close() {
        if (handle != 0) {
            Native.setDestroy(handle);
            handle = 0;
        }
    }
}
