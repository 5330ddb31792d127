/* The tests' side of tests/jni/fake_jvm.c: a JNIEnv over plain C objects that behaves like the strictest JVM the JNI
 * specification allows, and what a test needs to build arguments and to look at the outcome.  Not thread-safe. */
#ifndef NEEDLE_TESTS_FAKE_JVM_H
#define NEEDLE_TESTS_FAKE_JVM_H

#include <stddef.h>
#include <jni.h>

enum { FJ_BYTE = 1, FJ_CHAR = 2, FJ_SHORT = 3, FJ_INT = 4, FJ_LONG = 5, FJ_FLOAT = 6, FJ_OBJECT = 7, FJ_BUFFER = 8, FJ_STRING = 9, FJ_HEAP_BUFFER = 10 };

/* what the fake records as a fault; fj_fault_count(kind), kind < 0: all of them */
enum {
    FJ_F_UNKNOWN_RELEASE = 0, /* a release of a pointer that was never handed out */
    FJ_F_WRONG_RELEASE,       /* a release against another array or another element type */
    FJ_F_DOUBLE_RELEASE,      /* a second release of the same pointer */
    FJ_F_REGION,              /* Set / Get<T>ArrayRegion outside the array (also raises the pending exception) */
    FJ_F_NULL,                /* GetArrayLength / Get<T>ArrayElements / a region call / GetObjectArrayElement on NULL */
    FJ_F_NOT_DIRECT,          /* GetDirectBufferAddress on NULL or on something that is no java.nio.Buffer at all */
    FJ_F_SENTINEL,            /* the bytes in front of or behind a handed-out copy were changed */
    FJ_F_TYPE,                /* a call on an object of another kind (GetIntArrayElements of a long[], ...) */
    FJ_F_KINDS
};

JNIEnv *fj_env(void);
jobject fj_new_array(int kind, jsize length, const void *init); /* a primitive array; init: length elements or NULL (zeroes) */
jobject fj_new_object_array(jsize length, const jobject *elements);
jobject fj_new_direct_buffer(void *address, jlong capacity);    /* over the caller's memory, which must outlive it */
jobject fj_new_heap_buffer(void);                               /* a ByteBuffer.allocate(): GetDirectBufferAddress gives NULL, as specified */
jsize fj_array_length(jobject array);
size_t fj_array_bytes(jobject array);                            /* length * element size */
const void *fj_array_data(jobject array);                        /* the array's own storage (NOT what Get...Elements hands out) */
const char *fj_string_utf(jobject string);                       /* what NewStringUTF was given */
int fj_outstanding_pins(void);                                   /* Get...Elements not yet released (JNI_COMMIT does not release) */
int fj_fault_count(int kind);
const char *fj_fault_log(void);                                  /* "name=count ..." and the last fault's message; "" when there is none */
int fj_exception_pending(void);
void fj_clear_exception(void);                                  /* the native returned and Java code caught what was pending */
void fj_fail_gets(int skip, int count);                          /* after `skip` more Get...Elements calls, the next `count` return NULL */
int fj_fail_gets_left(void);                                     /* how many of those are still to come */
int fj_get_calls(void);                                          /* Get...Elements calls since the last reset */
void fj_reset(void);                                             /* frees every object, pin and log entry */

#endif
