/*
 * A fake JNIEnv for the tests of bindings/jni/needle_jni.c (see tests/jni/jni.h: NOT a JVM's table layout).
 *
 * It behaves like the strictest JVM the JNI specification allows: Get<T>ArrayElements always returns a COPY (isCopy
 * true) in a fresh allocation with 64 sentinel bytes in front and behind, so
 *   - what native code writes reaches the Java array only through a release with mode 0 or JNI_COMMIT,
 *   - JNI_ABORT throws it away,
 *   - a write one element outside the copy lands in a sentinel and is reported when the copy is released.
 * Everything the specification leaves undefined and a shim must therefore never do is recorded as a fault (fake_jvm.h).
 */
#include "fake_jvm.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define FJ_MAGIC 0x4A4F424Au
#define FJ_SENTINEL_BYTES 64
#define FJ_SENTINEL_BYTE 0xA5

struct _jobject {
    unsigned magic;
    int kind;
    jsize length;
    size_t elem;   /* element size (arrays) */
    void *data;    /* arrays and strings: own storage; direct buffers: the caller's memory */
    int owns;
    struct _jobject *next;
};

typedef struct fj_pin {
    struct _jobject *array;
    unsigned char *base; /* allocation: sentinel, copy, sentinel */
    size_t bytes;
    int released;
    struct fj_pin *next;
} fj_pin;

static struct _jobject *g_objects;
static fj_pin *g_pins;
static int g_faults[FJ_F_KINDS];
static char g_last[256];
static char g_log[640];
static int g_exception;
static int g_fail_skip, g_fail_count;
static int g_get_calls;

static const char *const k_fault_names[FJ_F_KINDS] = {"unknown_release", "wrong_release", "double_release", "region_out_of_bounds",
                                                      "null_argument",   "not_a_direct_buffer", "sentinel_damaged", "wrong_type"};
static const char *const k_kind_names[] = {"?", "byte[]", "char[]", "short[]", "int[]", "long[]", "float[]", "Object[]", "DirectByteBuffer", "String", "HeapByteBuffer"};

static void fault(int kind, const char *what, const char *detail) {
    g_faults[kind]++;
    snprintf(g_last, sizeof(g_last), "%s: %s%s%s", k_fault_names[kind], what, detail ? " " : "", detail ? detail : "");
}

static size_t elem_size(int kind) {
    switch (kind) {
    case FJ_BYTE: return 1;
    case FJ_CHAR: case FJ_SHORT: return 2;
    case FJ_INT: case FJ_FLOAT: return 4;
    case FJ_LONG: return 8;
    case FJ_OBJECT: return sizeof(jobject);
    default: return 0;
    }
}

static struct _jobject *new_object(int kind, jsize length, size_t bytes) {
    struct _jobject *o = (struct _jobject *)calloc(1, sizeof(*o));
    if (!o) abort();
    o->magic = FJ_MAGIC;
    o->kind = kind;
    o->length = length;
    o->elem = elem_size(kind);
    o->data = calloc(bytes ? bytes : 1, 1);
    if (!o->data) abort();
    o->owns = 1;
    o->next = g_objects;
    g_objects = o;
    return o;
}

static int is_array(const struct _jobject *o) { return o->kind >= FJ_BYTE && o->kind <= FJ_OBJECT; }

/* the object behind a reference when it is of the kind asked for (0: any array); records the fault otherwise */
static struct _jobject *checked(jobject ref, int kind, const char *call) {
    if (!ref) {
        fault(FJ_F_NULL, call, "on NULL");
        return NULL;
    }
    if (ref->magic != FJ_MAGIC) {
        fault(FJ_F_TYPE, call, "on something that is no object of this JVM");
        return NULL;
    }
    if (kind ? ref->kind != kind : !is_array(ref)) {
        fault(FJ_F_TYPE, call, k_kind_names[ref->kind]);
        return NULL;
    }
    return ref;
}

/* ---- the JNIEnv's functions ---- */

static jstring f_NewStringUTF(JNIEnv *env, const char *utf) {
    (void)env;
    if (!utf) {
        fault(FJ_F_NULL, "NewStringUTF", "of NULL");
        return NULL;
    }
    const size_t n = strlen(utf);
    struct _jobject *o = new_object(FJ_STRING, (jsize)n, n + 1);
    memcpy(o->data, utf, n + 1);
    return o;
}

static jsize f_GetArrayLength(JNIEnv *env, jarray array) {
    (void)env;
    struct _jobject *o = checked(array, 0, "GetArrayLength");
    return o ? o->length : 0;
}

static jboolean f_ExceptionCheck(JNIEnv *env) {
    (void)env;
    return g_exception ? JNI_TRUE : JNI_FALSE;
}

static jobject f_GetObjectArrayElement(JNIEnv *env, jobjectArray array, jsize index) {
    (void)env;
    struct _jobject *o = checked(array, FJ_OBJECT, "GetObjectArrayElement");
    if (!o) return NULL;
    if (index < 0 || index >= o->length) {
        fault(FJ_F_REGION, "GetObjectArrayElement", "index outside the array");
        g_exception = 1;
        return NULL;
    }
    return ((jobject *)o->data)[index];
}

static void *f_GetDirectBufferAddress(JNIEnv *env, jobject buf) {
    (void)env;
    if (buf && buf->magic == FJ_MAGIC && buf->kind == FJ_HEAP_BUFFER) return NULL; /* (a heap buffer: NULL is the specified answer) */
    if (!buf || buf->magic != FJ_MAGIC || buf->kind != FJ_BUFFER) {
        fault(FJ_F_NOT_DIRECT, "GetDirectBufferAddress", !buf ? "on NULL" : "on something that is no buffer");
        return NULL;
    }
    return buf->data;
}

static jbyteArray f_NewByteArray(JNIEnv *env, jsize len) {
    (void)env;
    if (len < 0) {
        fault(FJ_F_REGION, "NewByteArray", "of a negative length");
        g_exception = 1;
        return NULL;
    }
    return new_object(FJ_BYTE, len, (size_t)len);
}

static void *get_elements(jarray array, int kind, jboolean *is_copy, const char *call) {
    g_get_calls++;
    struct _jobject *o = checked(array, kind, call);
    if (!o) return NULL;
    if (g_fail_skip > 0) {
        g_fail_skip--;
    } else if (g_fail_count > 0) {
        g_fail_count--;
        g_exception = 1; /* an OutOfMemoryError is pending */
        return NULL;
    }
    fj_pin *p = (fj_pin *)calloc(1, sizeof(*p));
    if (!p) abort();
    p->array = o;
    p->bytes = (size_t)o->length * o->elem;
    p->base = (unsigned char *)malloc(p->bytes + 2 * FJ_SENTINEL_BYTES);
    if (!p->base) abort();
    memset(p->base, FJ_SENTINEL_BYTE, FJ_SENTINEL_BYTES);
    memcpy(p->base + FJ_SENTINEL_BYTES, o->data, p->bytes);
    memset(p->base + FJ_SENTINEL_BYTES + p->bytes, FJ_SENTINEL_BYTE, FJ_SENTINEL_BYTES);
    p->next = g_pins;
    g_pins = p;
    if (is_copy) *is_copy = JNI_TRUE;
    return p->base + FJ_SENTINEL_BYTES;
}

static void release_elements(jarray array, void *elems, jint mode, int kind, const char *call) {
    fj_pin *live = NULL, *dead = NULL;
    for (fj_pin *p = g_pins; p; p = p->next) {
        if (p->base + FJ_SENTINEL_BYTES != (unsigned char *)elems) continue;
        if (!p->released) {
            live = p;
            break;
        }
        if (!dead) dead = p;
    }
    if (!live) {
        if (dead) fault(FJ_F_DOUBLE_RELEASE, call, "of a pointer that was released before");
        else fault(FJ_F_UNKNOWN_RELEASE, call, elems ? "of a pointer this JVM never handed out" : "of NULL");
        return;
    }
    if (live->array != array || live->array->kind != kind) {
        fault(FJ_F_WRONG_RELEASE, call, live->array != array ? "against another array than the pointer came from" : "with another element type");
        return; /* (the copy stays outstanding: the pin count shows it too) */
    }
    if (mode != 0 && mode != JNI_COMMIT && mode != JNI_ABORT) {
        fault(FJ_F_WRONG_RELEASE, call, "with a mode that is none of 0, JNI_COMMIT, JNI_ABORT");
        return;
    }
    if (mode != JNI_COMMIT) {
        const unsigned char *front = live->base, *behind = live->base + FJ_SENTINEL_BYTES + live->bytes;
        for (int i = 0; i < FJ_SENTINEL_BYTES; i++) {
            if (front[i] != FJ_SENTINEL_BYTE || behind[i] != FJ_SENTINEL_BYTE) {
                fault(FJ_F_SENTINEL, call, front[i] != FJ_SENTINEL_BYTE ? "found bytes in FRONT of the elements overwritten" : "found bytes BEHIND the elements overwritten");
                break;
            }
        }
    }
    if (mode != JNI_ABORT) memcpy(live->array->data, live->base + FJ_SENTINEL_BYTES, live->bytes);
    if (mode != JNI_COMMIT) {
        free(live->base); /* (the record stays, so that a second release of the pointer is told from an unknown one) */
        live->released = 1;
        for (fj_pin *p = g_pins; p; p = p->next) /* the allocator may hand the address out again: older records of it go */
            if (p != live && p->released && p->base == live->base) p->base = NULL;
    }
}

#define ELEMENTS(T, K, ctype)                                                                                                \
    static ctype *f_Get##T##ArrayElements(JNIEnv *env, jarray a, jboolean *c) {                                               \
        (void)env;                                                                                                            \
        return (ctype *)get_elements(a, K, c, "Get" #T "ArrayElements");                                                      \
    }                                                                                                                         \
    static void f_Release##T##ArrayElements(JNIEnv *env, jarray a, ctype *e, jint mode) {                                      \
        (void)env;                                                                                                            \
        release_elements(a, e, mode, K, "Release" #T "ArrayElements");                                                        \
    }
ELEMENTS(Byte, FJ_BYTE, jbyte)
ELEMENTS(Char, FJ_CHAR, jchar)
ELEMENTS(Short, FJ_SHORT, jshort)
ELEMENTS(Int, FJ_INT, jint)
ELEMENTS(Long, FJ_LONG, jlong)

static void region(jarray array, int kind, jsize start, jsize len, void *to, const void *from, const char *call) {
    struct _jobject *o = checked(array, kind, call);
    if (!o) return;
    if (start < 0 || len < 0 || (jlong)start + len > o->length) {
        fault(FJ_F_REGION, call, "outside the array");
        g_exception = 1; /* ArrayIndexOutOfBoundsException */
        return;
    }
    if (!to && !from) {
        fault(FJ_F_NULL, call, "with a NULL buffer");
        return;
    }
    if (from) memcpy((char *)o->data + (size_t)start * o->elem, from, (size_t)len * o->elem);
    else memcpy(to, (const char *)o->data + (size_t)start * o->elem, (size_t)len * o->elem);
}

static void f_SetIntArrayRegion(JNIEnv *env, jintArray a, jsize s, jsize n, const jint *b) { (void)env; region(a, FJ_INT, s, n, NULL, b, "SetIntArrayRegion"); }
static void f_SetLongArrayRegion(JNIEnv *env, jlongArray a, jsize s, jsize n, const jlong *b) { (void)env; region(a, FJ_LONG, s, n, NULL, b, "SetLongArrayRegion"); }
static void f_SetFloatArrayRegion(JNIEnv *env, jfloatArray a, jsize s, jsize n, const jfloat *b) { (void)env; region(a, FJ_FLOAT, s, n, NULL, b, "SetFloatArrayRegion"); }
static void f_GetIntArrayRegion(JNIEnv *env, jintArray a, jsize s, jsize n, jint *b) { (void)env; region(a, FJ_INT, s, n, b, NULL, "GetIntArrayRegion"); }

static const struct JNINativeInterface_ k_table = {
    f_NewStringUTF,           f_GetArrayLength,          f_ExceptionCheck,           f_GetObjectArrayElement,  f_GetDirectBufferAddress,
    f_NewByteArray,           f_GetByteArrayElements,    f_GetCharArrayElements,     f_GetShortArrayElements,  f_GetIntArrayElements,
    f_GetLongArrayElements,   f_ReleaseByteArrayElements, f_ReleaseCharArrayElements, f_ReleaseShortArrayElements, f_ReleaseIntArrayElements,
    f_ReleaseLongArrayElements, f_SetIntArrayRegion,     f_SetLongArrayRegion,       f_SetFloatArrayRegion,    f_GetIntArrayRegion,
};
static const struct JNINativeInterface_ *g_env = &k_table;

/* ---- the tests' side ---- */

JNIEnv *fj_env(void) { return &g_env; }

jobject fj_new_array(int kind, jsize length, const void *init) {
    if (kind < FJ_BYTE || kind > FJ_FLOAT || length < 0) return NULL;
    struct _jobject *o = new_object(kind, length, (size_t)length * elem_size(kind));
    if (init) memcpy(o->data, init, (size_t)length * o->elem);
    return o;
}

jobject fj_new_object_array(jsize length, const jobject *elements) {
    if (length < 0) return NULL;
    struct _jobject *o = new_object(FJ_OBJECT, length, (size_t)length * sizeof(jobject));
    if (elements) memcpy(o->data, elements, (size_t)length * sizeof(jobject));
    return o;
}

jobject fj_new_direct_buffer(void *address, jlong capacity) {
    struct _jobject *o = new_object(FJ_BUFFER, (jsize)(capacity > 0x7FFFFFFF ? 0x7FFFFFFF : capacity), 0);
    free(o->data);
    o->data = address;
    o->owns = 0;
    return o;
}

jobject fj_new_heap_buffer(void) { return new_object(FJ_HEAP_BUFFER, 0, 0); }

jsize fj_array_length(jobject array) { return array && array->magic == FJ_MAGIC ? array->length : -1; }
size_t fj_array_bytes(jobject array) { return array && array->magic == FJ_MAGIC && is_array(array) ? (size_t)array->length * array->elem : 0; }
const void *fj_array_data(jobject array) { return array && array->magic == FJ_MAGIC && is_array(array) ? array->data : NULL; }
const char *fj_string_utf(jobject string) { return string && string->magic == FJ_MAGIC && string->kind == FJ_STRING ? (const char *)string->data : NULL; }

int fj_outstanding_pins(void) {
    int n = 0;
    for (fj_pin *p = g_pins; p; p = p->next) n += !p->released;
    return n;
}

int fj_fault_count(int kind) {
    if (kind >= 0) return kind < FJ_F_KINDS ? g_faults[kind] : 0;
    int n = 0;
    for (int i = 0; i < FJ_F_KINDS; i++) n += g_faults[i];
    return n;
}

const char *fj_fault_log(void) {
    size_t at = 0;
    g_log[0] = 0;
    if (!fj_fault_count(-1)) return g_log;
    for (int i = 0; i < FJ_F_KINDS; i++)
        if (g_faults[i]) at += (size_t)snprintf(g_log + at, sizeof(g_log) - at, "%s=%d ", k_fault_names[i], g_faults[i]);
    snprintf(g_log + at, sizeof(g_log) - at, "| last: %s", g_last);
    return g_log;
}

int fj_exception_pending(void) { return g_exception; }
void fj_clear_exception(void) { g_exception = 0; }

void fj_fail_gets(int skip, int count) {
    g_fail_skip = skip < 0 ? 0 : skip;
    g_fail_count = count < 0 ? 0 : count;
}

int fj_fail_gets_left(void) { return g_fail_count; }
int fj_get_calls(void) { return g_get_calls; }

void fj_reset(void) {
    while (g_pins) {
        fj_pin *p = g_pins;
        g_pins = p->next;
        if (!p->released) free(p->base);
        free(p);
    }
    while (g_objects) {
        struct _jobject *o = g_objects;
        g_objects = o->next;
        if (o->owns) free(o->data);
        o->magic = 0;
        free(o);
    }
    memset(g_faults, 0, sizeof(g_faults));
    g_last[0] = 0;
    g_exception = 0;
    g_fail_skip = g_fail_count = 0;
    g_get_calls = 0;
}
