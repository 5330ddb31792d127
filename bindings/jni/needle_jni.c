/*
 * JNI shim: com.justinblank.strings.gpu.Native -> libneedle_hip.so (include/needle_hip.h).
 * Thin by design: unpack Java arrays / direct buffers, call the C ABI, return its status code.  No exception is
 * raised here; GpuPattern.check() maps status codes to the reference's exception types.
 *
 * COMPILED AND EXERCISED AGAINST A STAND-IN jni.h AND A FAKE JNIEnv (tests/jni/, tests/test_jni_shim.py,
 * tests/test_gpu_jni_shim.py: every native, its argument checks, its releases, its results against the oracle);
 * NEVER LOADED BY A JVM: the build image has no JDK.  Build on a box with a JDK:
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude bindings/jni/needle_jni.c \
 *       -Lneedle_amd -lneedle_hip -o libneedle_jni.so
 *
 * The rules every native here keeps (the tests hold each of them to these):
 *   - a Java ARRAY the C ABI will dereference is checked first: not null, and long enough for what the header's contract
 *     reads or writes there -- a short array from the caller becomes NEEDLE_ERR_INVALID, never an access past it.
 *     Direct ByteBuffers are checked for null and for being direct, NOT for their capacity (see view_of);
 *   - Get<T>ArrayElements may return NULL (OutOfMemoryError pending): what was obtained is released unchanged and the
 *     native returns NEEDLE_ERR_INVALID;
 *   - a JVM may hand out COPIES: an array the library writes is released with mode 0 (copied back), one it only reads
 *     with JNI_ABORT; every obtained pointer is released exactly once, against its own array.
 */
#include <jni.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "needle_hip.h"

#define NATIVE(ret, name) JNIEXPORT ret JNICALL Java_com_justinblank_strings_gpu_Native_##name

/* n elements fit the Java array (a short array from the caller must not become an access past it) */
static int byte_room(JNIEnv *env, jbyteArray a, jlong n) { return a != NULL && (jlong)(*env)->GetArrayLength(env, a) >= n; }
static int short_room(JNIEnv *env, jshortArray a, jlong n) { return a != NULL && (jlong)(*env)->GetArrayLength(env, a) >= n; }
static int int_room(JNIEnv *env, jintArray a, jlong n) { return a != NULL && (jlong)(*env)->GetArrayLength(env, a) >= n; }
static int long_room(JNIEnv *env, jlongArray a, jlong n) { return a != NULL && (jlong)(*env)->GetArrayLength(env, a) >= n; }
static int float_room(JNIEnv *env, jfloatArray a, jlong n) { return a != NULL && (jlong)(*env)->GetArrayLength(env, a) >= n; }
/* an optional output: null (not wanted) or with room */
static int int_room_or_null(JNIEnv *env, jintArray a, jlong n) { return a == NULL || int_room(env, a, n); }
static int long_room_or_null(JNIEnv *env, jlongArray a, jlong n) { return a == NULL || long_room(env, a, n); }

/* The elements of the arrays one native holds.  pin(): Get<T>ArrayElements by element type ('B', 'C', 'S', 'I', 'J') with the mode
 * its release takes; NULL for a null array (an optional argument) and after a failure.  unpin(): releases every one, in reverse
 * order -- all with JNI_ABORT when a Get returned NULL, so that nothing half-written reaches the caller -- and gives the status. */
#define NEEDLE_JNI_MAX_PINS 8
typedef struct {
    JNIEnv *env;
    int n, failed;
    struct {
        jarray a;
        void *p;
        char t;
        jint mode;
    } e[NEEDLE_JNI_MAX_PINS];
} pins;

static void pins_init(pins *ps, JNIEnv *env) {
    ps->env = env;
    ps->n = ps->failed = 0;
}

static void *pin(pins *ps, jarray a, char t, jint mode) {
    JNIEnv *env = ps->env;
    if (!a || ps->failed) return NULL;
    if (ps->n == NEEDLE_JNI_MAX_PINS) {
        ps->failed = 1;
        return NULL;
    }
    void *p = t == 'B'   ? (void *)(*env)->GetByteArrayElements(env, a, NULL)
              : t == 'C' ? (void *)(*env)->GetCharArrayElements(env, a, NULL)
              : t == 'S' ? (void *)(*env)->GetShortArrayElements(env, a, NULL)
              : t == 'I' ? (void *)(*env)->GetIntArrayElements(env, a, NULL)
                         : (void *)(*env)->GetLongArrayElements(env, a, NULL);
    if (!p) {
        ps->failed = 1; /* OutOfMemoryError pending */
        return NULL;
    }
    ps->e[ps->n].a = a;
    ps->e[ps->n].p = p;
    ps->e[ps->n].t = t;
    ps->e[ps->n].mode = mode;
    ps->n++;
    return p;
}

static jint unpin(pins *ps, jint rc) {
    JNIEnv *env = ps->env;
    while (ps->n > 0) {
        ps->n--;
        jarray a = ps->e[ps->n].a;
        void *p = ps->e[ps->n].p;
        const jint mode = ps->failed ? JNI_ABORT : ps->e[ps->n].mode;
        switch (ps->e[ps->n].t) {
        case 'B': (*env)->ReleaseByteArrayElements(env, a, (jbyte *)p, mode); break;
        case 'C': (*env)->ReleaseCharArrayElements(env, a, (jchar *)p, mode); break;
        case 'S': (*env)->ReleaseShortArrayElements(env, a, (jshort *)p, mode); break;
        case 'I': (*env)->ReleaseIntArrayElements(env, a, (jint *)p, mode); break;
        default: (*env)->ReleaseLongArrayElements(env, a, (jlong *)p, mode); break;
        }
    }
    return ps->failed ? NEEDLE_ERR_INVALID : rc;
}

static void put_long(JNIEnv *env, jlongArray a, jlong v) { (*env)->SetLongArrayRegion(env, a, 0, 1, &v); }
static void put_int(JNIEnv *env, jintArray a, jint v) { (*env)->SetIntArrayRegion(env, a, 0, 1, &v); }

NATIVE(jstring, lastError)(JNIEnv *env, jclass c) { return (*env)->NewStringUTF(env, needle_last_error()); }
NATIVE(jint, deviceCount)(JNIEnv *env, jclass c) { return needle_device_count(); }

NATIVE(jint, compile)(JNIEnv *env, jclass c, jcharArray regex, jint flags, jlongArray out) {
    if (!regex || !long_room(env, out, 1)) return NEEDLE_ERR_INVALID;
    jsize n = (*env)->GetArrayLength(env, regex);
    pins ps;
    pins_init(&ps, env);
    jchar *u = (jchar *)pin(&ps, regex, 'C', JNI_ABORT);
    if (ps.failed) return unpin(&ps, 0);
    needle_pattern *p = NULL;
    int rc = needle_compile((const uint16_t *)u, (size_t)n, flags, &p);
    put_long(env, out, (jlong)(intptr_t)p);
    return unpin(&ps, rc);
}

NATIVE(jint, fromTables)(JNIEnv *env, jclass c, jbyteArray classMap, jint stride, jintArray nStates, jintArray maxChar,
                         jobjectArray tables, jobjectArray accepting, jint fixedLen, jlongArray out) {
    /* Everything the C ABI will read is checked against the Java arrays' real lengths first: needle_pattern_from_tables
     * copies n_states * stride shorts, n_states bytes and 65536 class-map bytes from raw pointers. */
    if (!classMap || !nStates || !maxChar || !tables || !accepting || !out) return NEEDLE_ERR_INVALID;
    if (!byte_room(env, classMap, 65536) || !int_room(env, nStates, 4) || !int_room(env, maxChar, 4) || (*env)->GetArrayLength(env, tables) < 4 ||
        (*env)->GetArrayLength(env, accepting) < 4 || !long_room(env, out, 1) || stride < 1 || stride > 255)
        return NEEDLE_ERR_INVALID;
    needle_table_desc d;
    memset(&d, 0, sizeof(d));
    jint ns[4], mc[4];
    (*env)->GetIntArrayRegion(env, nStates, 0, 4, ns);
    (*env)->GetIntArrayRegion(env, maxChar, 0, 4, mc);
    if ((*env)->ExceptionCheck(env)) return NEEDLE_ERR_INVALID;
    needle_dfa_desc *ds[4] = {&d.matches, &d.contained_in, &d.forwards, &d.backwards};
    jshortArray ta[4] = {0};
    jbyteArray aa[4] = {0};
    jshort *tp[4] = {0};
    jbyte *ap[4] = {0};
    jbyte *cm = NULL;
    int rc = NEEDLE_OK;
    for (int i = 0; i < 4 && rc == NEEDLE_OK; i++) {
        ta[i] = (jshortArray)(*env)->GetObjectArrayElement(env, tables, i);
        aa[i] = (jbyteArray)(*env)->GetObjectArrayElement(env, accepting, i);
        if (!ta[i] || !aa[i] || ns[i] < 1 || ns[i] > 16383 || !short_room(env, ta[i], (jlong)ns[i] * stride) || !byte_room(env, aa[i], ns[i]))
            rc = NEEDLE_ERR_INVALID;
    }
    if (rc == NEEDLE_OK && !(cm = (*env)->GetByteArrayElements(env, classMap, NULL))) rc = NEEDLE_ERR_INVALID;
    for (int i = 0; i < 4 && rc == NEEDLE_OK; i++) {
        tp[i] = (*env)->GetShortArrayElements(env, ta[i], NULL);
        if (tp[i]) ap[i] = (*env)->GetByteArrayElements(env, aa[i], NULL);
        if (!tp[i] || !ap[i]) rc = NEEDLE_ERR_INVALID; /* OutOfMemoryError pending */
        ds[i]->n_states = ns[i];
        ds[i]->max_char = mc[i];
        ds[i]->table = (const int16_t *)tp[i];
        ds[i]->accepting = (const uint8_t *)ap[i];
    }
    needle_pattern *p = NULL;
    const int called = rc == NEEDLE_OK;
    if (called) {
        d.class_map = (const uint8_t *)cm;
        d.stride = stride;
        d.fixed_len = fixedLen;
        rc = needle_pattern_from_tables(&d, &p); /* copies everything it needs */
    }
    for (int i = 0; i < 4; i++) {
        if (tp[i]) (*env)->ReleaseShortArrayElements(env, ta[i], tp[i], JNI_ABORT);
        if (ap[i]) (*env)->ReleaseByteArrayElements(env, aa[i], ap[i], JNI_ABORT);
    }
    if (cm) (*env)->ReleaseByteArrayElements(env, classMap, cm, JNI_ABORT);
    if (called) put_long(env, out, (jlong)(intptr_t)p); /* (an argument refused here leaves every array as it was) */
    return rc;
}

NATIVE(void, destroyPattern)(JNIEnv *env, jclass c, jlong h) { needle_pattern_destroy((needle_pattern *)(intptr_t)h); }

/* A fixed-stride host batch in direct buffers: rows is required, lengths may be null; neither may be a heap buffer
 * (GetDirectBufferAddress gives NULL for those).  0 when the view cannot be formed.
 * NOT checked: the buffers' CAPACITY.  rows must hold nRows * rowStride chars and lengths nRows ints -- that is the
 * caller's to keep; a shorter direct buffer is read past its end. */
static int view_of(JNIEnv *env, needle_batch_view *v, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths) {
    memset(v, 0, sizeof(*v));
    if (!rows || n < 0 || stride < 0 || rowLen < 0) return 0;
    v->rows = (*env)->GetDirectBufferAddress(env, rows);
    v->char_width = (uint32_t)cw;
    v->n_rows = (uint64_t)n;
    v->row_stride = (uint64_t)stride;
    v->row_len = (uint32_t)rowLen;
    v->lengths = lengths ? (const uint32_t *)(*env)->GetDirectBufferAddress(env, lengths) : NULL;
    return v->rows != NULL && (!lengths || v->lengths != NULL);
}

static jlong bitmap_words(jlong n) { return (n + 63) / 64; }

static jint bitmap_call(JNIEnv *env, int which, jlong h, needle_batch_view *v, jlongArray bitmap, jintArray start, jintArray end) {
    const jlong n = (jlong)v->n_rows;
    if (!long_room(env, bitmap, bitmap_words(n))) return NEEDLE_ERR_INVALID;
    if (which == 2 && (!int_room(env, start, n) || !int_room(env, end, n))) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    jlong *bm = (jlong *)pin(&ps, bitmap, 'J', 0);
    jint *s = which == 2 ? (jint *)pin(&ps, start, 'I', 0) : NULL;
    jint *e = which == 2 ? (jint *)pin(&ps, end, 'I', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    const needle_pattern *p = (const needle_pattern *)(intptr_t)h;
    int rc = which == 0 ? needle_matches_host(p, v, (uint64_t *)bm)
           : which == 1 ? needle_contained_in_host(p, v, (uint64_t *)bm)
                        : needle_find_host(p, v, (uint64_t *)bm, (int32_t *)s, (int32_t *)e);
    return unpin(&ps, rc);
}

NATIVE(jint, matchesHost)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jlongArray bitmap) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    return bitmap_call(env, 0, h, &v, bitmap, NULL, NULL);
}
NATIVE(jint, containedInHost)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jlongArray bitmap) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    return bitmap_call(env, 1, h, &v, bitmap, NULL, NULL);
}
NATIVE(jint, findHost)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jlongArray bitmap, jintArray start, jintArray end) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    return bitmap_call(env, 2, h, &v, bitmap, start, end);
}

/* needle_find_all_host: counts int[n]; start / end int[n * maxPerRow]; more int[1] or null. */
NATIVE(jint, findAllHost)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jint maxPerRow, jintArray counts, jintArray start, jintArray end, jintArray more) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    if (maxPerRow < 0 || !int_room(env, counts, n) || !int_room(env, start, n * (jlong)maxPerRow) || !int_room(env, end, n * (jlong)maxPerRow) ||
        !int_room_or_null(env, more, 1))
        return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    jint *cn = (jint *)pin(&ps, counts, 'I', 0);
    jint *st = (jint *)pin(&ps, start, 'I', 0);
    jint *en = (jint *)pin(&ps, end, 'I', 0);
    if (ps.failed) return unpin(&ps, 0);
    int m = 0;
    int rc = needle_find_all_host((const needle_pattern *)(intptr_t)h, &v, (uint32_t)maxPerRow, (uint32_t *)cn, (int32_t *)st, (int32_t *)en, &m);
    if (more) put_int(env, more, m);
    return unpin(&ps, rc);
}

/* needle_find_all_packed16_host: counts int[n]; startEnd int[n * maxPerRow]; more int[1] or null. */
NATIVE(jint, findAllPacked16Host)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jint maxPerRow, jintArray counts, jintArray startEnd, jintArray more) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    if (maxPerRow < 0 || !int_room(env, counts, n) || !int_room(env, startEnd, n * (jlong)maxPerRow) || !int_room_or_null(env, more, 1)) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    jint *cn = (jint *)pin(&ps, counts, 'I', 0);
    jint *se = (jint *)pin(&ps, startEnd, 'I', 0);
    if (ps.failed) return unpin(&ps, 0);
    int m = 0;
    int rc = needle_find_all_packed16_host((const needle_pattern *)(intptr_t)h, &v, (uint32_t)maxPerRow, (uint32_t *)cn, (uint32_t *)se, &m);
    if (more) put_int(env, more, m);
    return unpin(&ps, rc);
}

/* The room of a match list's start / end (/ masks) arrays: the shortest of them, 0 when any is null (count only). */
static jsize list_capacity(JNIEnv *env, jintArray a, jintArray b, jintArray c3, int three) {
    if (!a || !b || (three && !c3)) return 0;
    jsize cap = (*env)->GetArrayLength(env, a);
    if ((*env)->GetArrayLength(env, b) < cap) cap = (*env)->GetArrayLength(env, b);
    if (three && (*env)->GetArrayLength(env, c3) < cap) cap = (*env)->GetArrayLength(env, c3);
    return cap;
}

/* needle_find_all_csr_host: offsets long[nRows + 1]; start / end int[capacity] (may be null with capacity 0: count only);
 * total long[1]. */
NATIVE(jint, findAllCsrHost)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jlongArray offsets, jintArray start, jintArray end, jlongArray total) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    if (!long_room(env, offsets, n + 1) || !long_room(env, total, 1)) return NEEDLE_ERR_INVALID;
    const jsize cap = list_capacity(env, start, end, NULL, 0);
    pins ps;
    pins_init(&ps, env);
    jlong *of = (jlong *)pin(&ps, offsets, 'J', 0);
    jint *st = cap ? (jint *)pin(&ps, start, 'I', 0) : NULL;
    jint *en = cap ? (jint *)pin(&ps, end, 'I', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    uint64_t t = 0;
    int rc = needle_find_all_csr_host((const needle_pattern *)(intptr_t)h, &v, (uint64_t *)of, (int32_t *)st, (int32_t *)en, (uint64_t)cap, &t);
    put_long(env, total, (jlong)t);
    return unpin(&ps, rc);
}

/* needle_find_compact_host: bitmap long[ceil(n / 64)]; records int[2 * cap] = needle_match_rec[cap] (may be null: count only);
 * nMatched long[1]. */
NATIVE(jint, findCompactHost)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jlongArray bitmap, jintArray records, jlongArray nMatched) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    if (!long_room(env, bitmap, bitmap_words(n)) || !long_room(env, nMatched, 1)) return NEEDLE_ERR_INVALID;
    const jsize cap = records ? (*env)->GetArrayLength(env, records) / 2 : 0;
    pins ps;
    pins_init(&ps, env);
    jlong *bm = (jlong *)pin(&ps, bitmap, 'J', 0);
    jint *rec = cap ? (jint *)pin(&ps, records, 'I', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    uint64_t m = 0;
    int rc = needle_find_compact_host((const needle_pattern *)(intptr_t)h, &v, (uint64_t *)bm, (needle_match_rec *)rec, (uint64_t)cap, &m);
    put_long(env, nMatched, (jlong)m);
    return unpin(&ps, rc);
}

/* needle_find_packed16_host: ONE int per row (start | end << 16; 0xFFFFFFFF: no match); rows of at most 65 534 chars */
NATIVE(jint, findPacked16Host)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jlongArray bitmap, jintArray startEnd) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    if (!long_room(env, bitmap, bitmap_words(n)) || !int_room(env, startEnd, n)) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    jlong *bm = (jlong *)pin(&ps, bitmap, 'J', 0);
    jint *se = (jint *)pin(&ps, startEnd, 'I', 0);
    if (ps.failed) return unpin(&ps, 0);
    return unpin(&ps, needle_find_packed16_host((const needle_pattern *)(intptr_t)h, &v, (uint64_t *)bm, (uint32_t *)se));
}

/* needle_find_packed8_host: rows of at most 256 chars, ONE short per row (start | (end - start) << 8; 0xFFFF: no match, 0xFFFE: (0, 256)) */
NATIVE(jint, findPacked8Host)(JNIEnv *env, jclass c, jlong h, jobject rows, jint cw, jlong n, jlong stride, jint rowLen, jobject lengths, jlongArray bitmap, jshortArray startLen) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    if (!long_room(env, bitmap, bitmap_words(n)) || !short_room(env, startLen, n)) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    jlong *bm = (jlong *)pin(&ps, bitmap, 'J', 0);
    jshort *sl = (jshort *)pin(&ps, startLen, 'S', 0);
    if (ps.failed) return unpin(&ps, 0);
    return unpin(&ps, needle_find_packed8_host((const needle_pattern *)(intptr_t)h, &v, (uint64_t *)bm, (uint16_t *)sl));
}

NATIVE(jstring, tuningInfo)(JNIEnv *env, jclass c) {
    size_t need = 0;
    if (needle_tuning_info(NULL, 0, &need) != NEEDLE_OK || need == 0) return (*env)->NewStringUTF(env, "");
    char *buf = (char *)malloc(need);
    if (!buf) return (*env)->NewStringUTF(env, "");
    (void)needle_tuning_info(buf, need, NULL);
    jstring s = (*env)->NewStringUTF(env, buf);
    free(buf);
    return s;
}

NATIVE(jint, trimScratch)(JNIEnv *env, jclass c, jlong keepBytes) { return needle_trim_scratch(keepBytes < 0 ? 0 : (size_t)keepBytes); }

/* needle_pattern_prefilter_info: info int[7] or null (not wanted); a shorter info: a null String */
NATIVE(jstring, prefilterInfo)(JNIEnv *env, jclass c, jlong h, jint which, jintArray info) {
    needle_prefilter_info pi;
    if (!int_room_or_null(env, info, 7)) return NULL;
    if (needle_pattern_prefilter_info((const needle_pattern *)(intptr_t)h, which, &pi, NULL) != NEEDLE_OK) return (*env)->NewStringUTF(env, needle_last_error());
    if (info) {
        const jint v[7] = {pi.on, pi.mode, pi.stride, pi.warm, pi.min_len, pi.n_windows, pi.bitmap_bytes};
        (*env)->SetIntArrayRegion(env, info, 0, 7, v);
    }
    return (*env)->NewStringUTF(env, pi.why);
}

/* needle_pattern_set_prefilter / needle_pattern_prefilter_state: the filter's flood watch pinned and reported (include/needle_hip.h).
 * state[0..3] = mode, has_filter, suspended_calls_left, backoff; rate[0] = last candidates per KiB; counts[0..1] = launches, suspended calls;
 * each may be null (not wanted). */
NATIVE(jint, setPrefilter)(JNIEnv *env, jclass c, jlong h, jint mode) { return needle_pattern_set_prefilter((needle_pattern *)(intptr_t)h, mode); }

NATIVE(jint, prefilterState)(JNIEnv *env, jclass c, jlong h, jint which, jintArray state, jfloatArray rate, jlongArray counts) {
    if (!int_room_or_null(env, state, 4) || (rate && !float_room(env, rate, 1)) || !long_room_or_null(env, counts, 2)) return NEEDLE_ERR_INVALID;
    needle_prefilter_state st;
    const int rc = needle_pattern_prefilter_state((const needle_pattern *)(intptr_t)h, which, &st);
    if (rc != NEEDLE_OK) return rc;
    if (state) {
        const jint v[4] = {st.mode, st.has_filter, st.suspended_calls_left, st.backoff};
        (*env)->SetIntArrayRegion(env, state, 0, 4, v);
    }
    if (rate) {
        const jfloat r = st.last_candidates_per_kib;
        (*env)->SetFloatArrayRegion(env, rate, 0, 1, &r);
    }
    if (counts) {
        const jlong v[2] = {(jlong)st.filter_launches, (jlong)st.suspended_calls};
        (*env)->SetLongArrayRegion(env, counts, 0, 2, v);
    }
    return NEEDLE_OK;
}

/* needle_pattern_find_all_packed_filter: out[0] = 1 when the packed find-all entries take the filter kernel for this pattern */
NATIVE(jint, findAllPackedFilter)(JNIEnv *env, jclass c, jlong h, jint charWidth, jint countOnly, jintArray out) {
    if (!int_room(env, out, 1)) return NEEDLE_ERR_INVALID;
    int32_t available = 0;
    const int rc = needle_pattern_find_all_packed_filter((const needle_pattern *)(intptr_t)h, charWidth, countOnly, &available);
    if (rc != NEEDLE_OK) return rc;
    put_int(env, out, available);
    return NEEDLE_OK;
}

/* needle_pattern_utf16_route: out[0] = page (-1: none), out[1] = substitute byte */
NATIVE(jint, utf16Route)(JNIEnv *env, jclass c, jlong h, jintArray out) {
    if (!int_room(env, out, 2)) return NEEDLE_ERR_INVALID;
    int32_t page = -1, sub = 0;
    const int rc = needle_pattern_utf16_route((const needle_pattern *)(intptr_t)h, &page, &sub);
    if (rc != NEEDLE_OK) return rc;
    const jint v[2] = {page, sub};
    (*env)->SetIntArrayRegion(env, out, 0, 2, v);
    return NEEDLE_OK;
}

/* A packed host batch: data (char[]: UTF-16 code units, or byte[]: UTF-8 bytes) + offsets long[n + 1].
 * packed_rows(): the number of rows, -1 when either array is null or offsets is empty (the checks before anything is pinned).
 * packed_view(): pins both read-only and fills v; the offsets' ends must lie inside data (the library checks that they ascend),
 * otherwise -- and when a Get gives NULL -- ps->failed is set. */
static jlong packed_rows(JNIEnv *env, jarray data, jlongArray offsets) {
    if (!data || !offsets) return -1;
    return (jlong)(*env)->GetArrayLength(env, offsets) - 1; /* (empty offsets: -1) */
}

static void packed_view(pins *ps, needle_packed_view *v, jarray data, int char_width, jlongArray offsets, jlong n) {
    JNIEnv *env = ps->env;
    memset(v, 0, sizeof(*v));
    const jlong *o = (const jlong *)pin(ps, offsets, 'J', JNI_ABORT);
    const void *d = pin(ps, data, char_width == 2 ? 'C' : 'B', JNI_ABORT);
    if (ps->failed) return;
    if (o[0] < 0 || o[n] < o[0] || o[n] > (jlong)(*env)->GetArrayLength(env, data)) {
        ps->failed = 1;
        return;
    }
    v->data = d;
    v->char_width = (uint32_t)char_width;
    v->n_rows = (uint64_t)n;
    v->offsets = (const uint64_t *)o;
}

/* needle_matches / contained_in / find_packed_host: op 0 | 1 | 2; bitmap long[(n + 63) / 64]; start / end int[n] for op 2 (not looked at
 * otherwise). */
NATIVE(jint, packedHost)(JNIEnv *env, jclass c, jlong h, jint op, jcharArray data, jlongArray offsets, jlongArray bitmap, jintArray start, jintArray end) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || op < 0 || op > 2 || !long_room(env, bitmap, bitmap_words(n))) return NEEDLE_ERR_INVALID;
    if (op == 2 && (!int_room(env, start, n) || !int_room(env, end, n))) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 2, offsets, n);
    jlong *bm = (jlong *)pin(&ps, bitmap, 'J', 0);
    jint *st = op == 2 ? (jint *)pin(&ps, start, 'I', 0) : NULL;
    jint *en = op == 2 ? (jint *)pin(&ps, end, 'I', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    const needle_pattern *p = (const needle_pattern *)(intptr_t)h;
    int rc = op == 0   ? needle_matches_packed_host(p, &v, (uint64_t *)bm)
             : op == 1 ? needle_contained_in_packed_host(p, &v, (uint64_t *)bm)
                       : needle_find_packed_host(p, &v, (uint64_t *)bm, (int32_t *)st, (int32_t *)en);
    return unpin(&ps, rc);
}

/* needle_find_all_csr_packed_host: data + offsets as packedHost; matchOffsets long[n + 1]; start / end int[capacity] (may be null:
 * count only); total long[1]. */
NATIVE(jint, findAllPackedHost)(JNIEnv *env, jclass c, jlong h, jcharArray data, jlongArray offsets, jlongArray matchOffsets, jintArray start, jintArray end, jlongArray total) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || !long_room(env, matchOffsets, n + 1) || !long_room(env, total, 1)) return NEEDLE_ERR_INVALID;
    const jsize cap = list_capacity(env, start, end, NULL, 0);
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 2, offsets, n);
    jlong *mo = (jlong *)pin(&ps, matchOffsets, 'J', 0);
    jint *st = cap ? (jint *)pin(&ps, start, 'I', 0) : NULL;
    jint *en = cap ? (jint *)pin(&ps, end, 'I', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    uint64_t t = 0;
    int rc = needle_find_all_csr_packed_host((const needle_pattern *)(intptr_t)h, &v, (uint64_t *)mo, (int32_t *)st, (int32_t *)en, (uint64_t)cap, &t);
    put_long(env, total, (jlong)t);
    return unpin(&ps, rc);
}

/* needle_find_all_csr_utf8_packed_host: data byte[] (the rows' UTF-8 bytes back to back) + offsets long[n + 1]; matchOffsets long[n + 1];
 * start / end int[capacity] (may be null: count only), BYTE offsets into the row; total long[1]; malformed long[(n + 63) / 64] or null. */
NATIVE(jint, findAllUtf8PackedHost)(JNIEnv *env, jclass c, jlong h, jbyteArray data, jlongArray offsets, jlongArray matchOffsets, jintArray start, jintArray end, jlongArray total, jlongArray malformed) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || !long_room(env, matchOffsets, n + 1) || !long_room(env, total, 1) || !long_room_or_null(env, malformed, bitmap_words(n))) return NEEDLE_ERR_INVALID;
    const jsize cap = list_capacity(env, start, end, NULL, 0);
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 1, offsets, n);
    jlong *mo = (jlong *)pin(&ps, matchOffsets, 'J', 0);
    jint *st = cap ? (jint *)pin(&ps, start, 'I', 0) : NULL;
    jint *en = cap ? (jint *)pin(&ps, end, 'I', 0) : NULL;
    jlong *ml = (jlong *)pin(&ps, malformed, 'J', 0);
    if (ps.failed) return unpin(&ps, 0);
    uint64_t t = 0;
    int rc = needle_find_all_csr_utf8_packed_host((const needle_pattern *)(intptr_t)h, &v, (uint64_t *)mo, (int32_t *)st, (int32_t *)en, (uint64_t)cap, &t,
                                                  (uint64_t *)ml);
    put_long(env, total, (jlong)t);
    return unpin(&ps, rc);
}

/* needle_contained_in_utf8_packed_host: data + offsets as findAllUtf8PackedHost; bitmap long[(n + 63) / 64]; malformed the same, or null. */
NATIVE(jint, containedInUtf8PackedHost)(JNIEnv *env, jclass c, jlong h, jbyteArray data, jlongArray offsets, jlongArray bitmap, jlongArray malformed) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || !long_room(env, bitmap, bitmap_words(n)) || !long_room_or_null(env, malformed, bitmap_words(n))) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 1, offsets, n);
    jlong *bm = (jlong *)pin(&ps, bitmap, 'J', 0);
    jlong *ml = (jlong *)pin(&ps, malformed, 'J', 0);
    if (ps.failed) return unpin(&ps, 0);
    return unpin(&ps, needle_contained_in_utf8_packed_host((const needle_pattern *)(intptr_t)h, &v, (uint64_t *)bm, (uint64_t *)ml));
}

/* needle_replace_all_packed_host: data + offsets as packedHost; replacement char[] (may be empty, not null); outOffsets long[n + 1];
 * out char[capacity] (may be null: size only); total long[1]. */
NATIVE(jint, replaceAllPackedHost)(JNIEnv *env, jclass c, jlong h, jcharArray data, jlongArray offsets, jcharArray replacement, jlongArray outOffsets, jcharArray out, jlongArray total) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || !replacement || !long_room(env, outOffsets, n + 1) || !long_room(env, total, 1)) return NEEDLE_ERR_INVALID;
    const jsize cap = out ? (*env)->GetArrayLength(env, out) : 0;
    const jsize rn = (*env)->GetArrayLength(env, replacement);
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 2, offsets, n);
    jchar *r = (jchar *)pin(&ps, replacement, 'C', JNI_ABORT);
    jlong *oo = (jlong *)pin(&ps, outOffsets, 'J', 0);
    jchar *text = cap ? (jchar *)pin(&ps, out, 'C', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    uint64_t t = 0;
    int rc = needle_replace_all_packed_host((const needle_pattern *)(intptr_t)h, &v, rn ? (const void *)r : NULL, (uint32_t)rn, (uint64_t *)oo, text,
                                            (uint64_t)cap, &t);
    put_long(env, total, (jlong)t);
    return unpin(&ps, rc);
}

/* needle_gather_matches_packed_host: data + offsets as packedHost; mode 0 (the matches) | 1 (the pieces between them); spanOffsets
 * long[n + 1]; outOffsets long[spanCapacity + 1] and out char[unitCapacity] (each may be null: size only); totals long[2]: output rows,
 * code units. */
NATIVE(jint, gatherMatchesPackedHost)(JNIEnv *env, jclass c, jlong h, jcharArray data, jlongArray offsets, jint mode, jlongArray spanOffsets, jlongArray outOffsets, jcharArray out, jlongArray totals) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || !long_room(env, spanOffsets, n + 1) || !long_room(env, totals, 2)) return NEEDLE_ERR_INVALID;
    const jsize span_cap = outOffsets && (*env)->GetArrayLength(env, outOffsets) > 0 ? (*env)->GetArrayLength(env, outOffsets) - 1 : 0;
    const jsize cap = out ? (*env)->GetArrayLength(env, out) : 0;
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 2, offsets, n);
    jlong *so = (jlong *)pin(&ps, spanOffsets, 'J', 0);
    jlong *oo = span_cap ? (jlong *)pin(&ps, outOffsets, 'J', 0) : NULL;
    jchar *text = cap ? (jchar *)pin(&ps, out, 'C', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    uint64_t ts = 0, tu = 0;
    int rc = needle_gather_matches_packed_host((const needle_pattern *)(intptr_t)h, &v, (int)mode, (uint64_t *)so, (uint64_t *)oo, (uint64_t)span_cap, text,
                                               (uint64_t)cap, &ts, &tu);
    const jlong jt[2] = {(jlong)ts, (jlong)tu};
    (*env)->SetLongArrayRegion(env, totals, 0, 2, jt);
    return unpin(&ps, rc);
}

/* needle_find_packed16_packed_host / needle_find_packed8_packed_host: data + offsets as packedHost; bitmap long[(n + 63) / 64];
 * the results int[n] (16) or short[n] (8). */
static jint find_packed_compact_host(JNIEnv *env, jlong h, jcharArray data, jlongArray offsets, jlongArray bitmap, jarray out, int bits) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || !long_room(env, bitmap, bitmap_words(n)) || !(bits == 16 ? int_room(env, out, n) : short_room(env, out, n))) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 2, offsets, n);
    jlong *bm = (jlong *)pin(&ps, bitmap, 'J', 0);
    void *r = pin(&ps, out, bits == 16 ? 'I' : 'S', 0);
    if (ps.failed) return unpin(&ps, 0);
    const needle_pattern *p = (const needle_pattern *)(intptr_t)h;
    int rc = bits == 16 ? needle_find_packed16_packed_host(p, &v, (uint64_t *)bm, (uint32_t *)r) : needle_find_packed8_packed_host(p, &v, (uint64_t *)bm, (uint16_t *)r);
    return unpin(&ps, rc);
}

NATIVE(jint, findPacked16PackedHost)(JNIEnv *env, jclass c, jlong h, jcharArray data, jlongArray offsets, jlongArray bitmap, jintArray startEnd) {
    return find_packed_compact_host(env, h, data, offsets, bitmap, startEnd, 16);
}

NATIVE(jint, findPacked8PackedHost)(JNIEnv *env, jclass c, jlong h, jcharArray data, jlongArray offsets, jlongArray bitmap, jshortArray startLen) {
    return find_packed_compact_host(env, h, data, offsets, bitmap, startLen, 8);
}

/* Pattern sets: needle_pattern_set_create / _destroy and the two packed host entries (op 0 matches, 1 containedIn); masks int[n]. */
NATIVE(jint, setCreate)(JNIEnv *env, jclass c, jlongArray patterns, jlongArray out) {
    if (!patterns || !long_room(env, out, 1)) return NEEDLE_ERR_INVALID;
    const jsize n = (*env)->GetArrayLength(env, patterns);
    if (n < 1 || n > NEEDLE_SET_MAX_PATTERNS) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    const jlong *h = (const jlong *)pin(&ps, patterns, 'J', JNI_ABORT);
    if (ps.failed) return unpin(&ps, 0);
    const needle_pattern *pp[NEEDLE_SET_MAX_PATTERNS];
    for (jsize i = 0; i < n; ++i) pp[i] = (const needle_pattern *)(intptr_t)h[i];
    needle_pattern_set *s = NULL;
    int rc = needle_pattern_set_create(pp, (int)n, &s);
    put_long(env, out, (jlong)(intptr_t)s);
    return unpin(&ps, rc);
}

NATIVE(void, setDestroy)(JNIEnv *env, jclass c, jlong s) { needle_pattern_set_destroy((needle_pattern_set *)(intptr_t)s); }

NATIVE(jint, setPackedHost)(JNIEnv *env, jclass c, jlong s, jint op, jcharArray data, jlongArray offsets, jintArray masks) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || (op != 0 && op != 1) || !int_room(env, masks, n)) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 2, offsets, n);
    jint *m = (jint *)pin(&ps, masks, 'I', 0);
    if (ps.failed) return unpin(&ps, 0);
    const needle_pattern_set *set = (const needle_pattern_set *)(intptr_t)s;
    int rc = op == 0 ? needle_set_matches_packed_host(set, &v, (uint32_t *)m) : needle_set_contained_in_packed_host(set, &v, (uint32_t *)m);
    return unpin(&ps, rc);
}

/* needle_set_tag_matches_packed_host: as findAllPackedHost, masks beside start / end (any of the three null: count only). */
NATIVE(jint, setTagMatchesPackedHost)(JNIEnv *env, jclass c, jlong s, jlong h, jcharArray data, jlongArray offsets, jlongArray matchOffsets,
                                      jintArray start, jintArray end, jintArray masks, jlongArray total) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || !long_room(env, matchOffsets, n + 1) || !long_room(env, total, 1)) return NEEDLE_ERR_INVALID;
    const jsize cap = list_capacity(env, start, end, masks, 1);
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 2, offsets, n);
    jlong *mo = (jlong *)pin(&ps, matchOffsets, 'J', 0);
    jint *st = cap ? (jint *)pin(&ps, start, 'I', 0) : NULL;
    jint *en = cap ? (jint *)pin(&ps, end, 'I', 0) : NULL;
    jint *mk = cap ? (jint *)pin(&ps, masks, 'I', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    uint64_t t = 0;
    int rc = needle_set_tag_matches_packed_host((const needle_pattern_set *)(intptr_t)s, (const needle_pattern *)(intptr_t)h, &v, (uint64_t *)mo,
                                                (int32_t *)st, (int32_t *)en, (uint32_t *)mk, (uint64_t)cap, &t);
    put_long(env, total, (jlong)t);
    return unpin(&ps, rc);
}

/* needle_set_replace_each_packed_host: data + offsets as packedHost; replacements char[] (may be empty, not null) located by
 * replOffsets int[nPatterns + 1]; outOffsets long[n + 1]; out char[capacity] (may be null: size only); total long[1]. */
NATIVE(jint, setReplaceEachPackedHost)(JNIEnv *env, jclass c, jlong s, jlong h, jcharArray data, jlongArray offsets, jcharArray replacements,
                                       jintArray replOffsets, jlongArray outOffsets, jcharArray out, jlongArray total) {
    const jlong n = packed_rows(env, data, offsets);
    if (n < 0 || !replacements || !int_room(env, replOffsets, 2) || !long_room(env, outOffsets, n + 1) || !long_room(env, total, 1)) return NEEDLE_ERR_INVALID;
    const jsize k1 = (*env)->GetArrayLength(env, replOffsets);
    const jsize cap = out ? (*env)->GetArrayLength(env, out) : 0;
    const jsize rn = (*env)->GetArrayLength(env, replacements);
    pins ps;
    pins_init(&ps, env);
    needle_packed_view v;
    packed_view(&ps, &v, data, 2, offsets, n);
    const jint *ro = (const jint *)pin(&ps, replOffsets, 'I', JNI_ABORT);
    /* (the table must lie inside the array; the entry checks the rest) */
    if (!ps.failed && (ro[0] != 0 || ro[k1 - 1] < 0 || ro[k1 - 1] > rn)) ps.failed = 1;
    jchar *r = (jchar *)pin(&ps, replacements, 'C', JNI_ABORT);
    jlong *oo = (jlong *)pin(&ps, outOffsets, 'J', 0);
    jchar *text = cap ? (jchar *)pin(&ps, out, 'C', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    uint64_t t = 0;
    int rc = needle_set_replace_each_packed_host((const needle_pattern_set *)(intptr_t)s, (const needle_pattern *)(intptr_t)h, &v,
                                                 rn ? (const void *)r : NULL, (const uint32_t *)ro, (uint32_t)(k1 - 1), (uint64_t *)oo, text,
                                                 (uint64_t)cap, &t);
    put_long(env, total, (jlong)t);
    return unpin(&ps, rc);
}

/* needle_set_matches_spans_packed_dev: device addresses as jlong. */
NATIVE(jint, setMatchesSpansPackedDev)(JNIEnv *env, jclass c, jlong s, jlong data, jint charWidth, jlong nRows, jlong offsets, jlong spanOffsets,
                                       jlong start, jlong end, jlong masks, jlong stream) {
    (void)env;
    if (nRows < 0) return NEEDLE_ERR_INVALID;
    needle_packed_view v;
    memset(&v, 0, sizeof(v));
    v.data = (const void *)(intptr_t)data;
    v.char_width = (uint32_t)charWidth;
    v.n_rows = (uint64_t)nRows;
    v.offsets = (const uint64_t *)(intptr_t)offsets;
    return needle_set_matches_spans_packed_dev((const needle_pattern_set *)(intptr_t)s, &v, (const uint64_t *)(intptr_t)spanOffsets,
                                               (const int32_t *)(intptr_t)start, (const int32_t *)(intptr_t)end, (uint32_t *)(intptr_t)masks,
                                               (void *)(intptr_t)stream);
}

NATIVE(jbyteArray, serialize)(JNIEnv *env, jclass c, jlong h) {
    size_t need = 0;
    const needle_pattern *p = (const needle_pattern *)(intptr_t)h;
    if (needle_pattern_serialize(p, NULL, 0, &need) != NEEDLE_OK || need > 0x7FFFFFFF) return NULL;
    jbyteArray out = (*env)->NewByteArray(env, (jsize)need);
    if (!out) return NULL;
    pins ps;
    pins_init(&ps, env);
    jbyte *b = (jbyte *)pin(&ps, out, 'B', 0);
    if (ps.failed) return NULL;
    return unpin(&ps, needle_pattern_serialize(p, b, need, &need)) == NEEDLE_OK ? out : NULL;
}

NATIVE(jint, deserialize)(JNIEnv *env, jclass c, jbyteArray blob, jlongArray out) {
    if (!blob || !long_room(env, out, 1)) return NEEDLE_ERR_INVALID;
    jsize n = (*env)->GetArrayLength(env, blob);
    pins ps;
    pins_init(&ps, env);
    jbyte *b = (jbyte *)pin(&ps, blob, 'B', JNI_ABORT);
    if (ps.failed) return unpin(&ps, 0);
    needle_pattern *p = NULL;
    int rc = needle_pattern_deserialize(b, (size_t)n, &p); /* validates every length and value itself */
    put_long(env, out, (jlong)(intptr_t)p);
    return unpin(&ps, rc);
}

NATIVE(jint, multiCreate)(JNIEnv *env, jclass c, jintArray devices, jint flags, jlongArray out) {
    if (!devices || !long_room(env, out, 1)) return NEEDLE_ERR_INVALID;
    jsize n = (*env)->GetArrayLength(env, devices);
    pins ps;
    pins_init(&ps, env);
    jint *d = (jint *)pin(&ps, devices, 'I', JNI_ABORT);
    if (ps.failed) return unpin(&ps, 0);
    needle_multi *m = NULL;
    int rc = needle_multi_create((const int *)d, (int)n, (unsigned)flags, &m);
    put_long(env, out, (jlong)(intptr_t)m);
    return unpin(&ps, rc);
}
NATIVE(void, multiDestroy)(JNIEnv *env, jclass c, jlong m) { needle_multi_destroy((needle_multi *)(intptr_t)m); }

NATIVE(jint, scanHostMulti)(JNIEnv *env, jclass c, jlong m, jlong h, jint op, jobject rows, jint cw, jlong n, jlong stride, jint rowLen,
                            jobject lengths, jlongArray bitmap, jintArray start, jintArray end) {
    needle_batch_view v;
    if (!view_of(env, &v, rows, cw, n, stride, rowLen, lengths)) return NEEDLE_ERR_INVALID;
    if (op < 0 || op > 2 || !long_room(env, bitmap, bitmap_words(n))) return NEEDLE_ERR_INVALID;
    if (op == 2 && (!int_room(env, start, n) || !int_room(env, end, n))) return NEEDLE_ERR_INVALID;
    pins ps;
    pins_init(&ps, env);
    jlong *bm = (jlong *)pin(&ps, bitmap, 'J', 0);
    jint *s = op == 2 ? (jint *)pin(&ps, start, 'I', 0) : NULL;
    jint *e = op == 2 ? (jint *)pin(&ps, end, 'I', 0) : NULL;
    if (ps.failed) return unpin(&ps, 0);
    return unpin(&ps, needle_scan_host_multi((needle_multi *)(intptr_t)m, (const needle_pattern *)(intptr_t)h, op, &v, (uint64_t *)bm, (int32_t *)s, (int32_t *)e));
}

NATIVE(jint, matcherCreate)(JNIEnv *env, jclass c, jlong pattern, jcharArray s, jlongArray out) {
    if (!s || !long_room(env, out, 1)) return NEEDLE_ERR_INVALID;
    jsize n = (*env)->GetArrayLength(env, s);
    pins ps;
    pins_init(&ps, env);
    jchar *u = (jchar *)pin(&ps, s, 'C', JNI_ABORT);
    if (ps.failed) return unpin(&ps, 0);
    needle_matcher *m = NULL;
    int rc = needle_matcher_create((const needle_pattern *)(intptr_t)pattern, (const uint16_t *)u, (size_t)n, &m);
    put_long(env, out, (jlong)(intptr_t)m);
    return unpin(&ps, rc);
}
NATIVE(void, matcherDestroy)(JNIEnv *env, jclass c, jlong m) { needle_matcher_destroy((needle_matcher *)(intptr_t)m); }

#define BOOL_CALL(jname, cname)                                                        \
    NATIVE(jint, jname)(JNIEnv *env, jclass c, jlong m, jintArray r) {                 \
        if (!int_room(env, r, 1)) return NEEDLE_ERR_INVALID;                           \
        int v = 0;                                                                     \
        int rc = cname((needle_matcher *)(intptr_t)m, &v);                             \
        put_int(env, r, v);                                                            \
        return rc;                                                                     \
    }
BOOL_CALL(matcherMatches, needle_matcher_matches)
BOOL_CALL(matcherContainedIn, needle_matcher_contained_in)
BOOL_CALL(matcherFind, needle_matcher_find)

NATIVE(jint, matcherFindRange)(JNIEnv *env, jclass c, jlong m, jint from, jint to, jintArray r) {
    if (!int_room(env, r, 1)) return NEEDLE_ERR_INVALID;
    int v = 0;
    int rc = needle_matcher_find_range((needle_matcher *)(intptr_t)m, from, to, &v);
    put_int(env, r, v);
    return rc;
}
NATIVE(jint, matcherStart)(JNIEnv *env, jclass c, jlong m) { return needle_matcher_start((const needle_matcher *)(intptr_t)m); }
NATIVE(jint, matcherEnd)(JNIEnv *env, jclass c, jlong m) { return needle_matcher_end((const needle_matcher *)(intptr_t)m); }
